"""pli_search_by_projection_reloc on the MI355X (the product library): relocalisation's ORBmatcher::SearchByProjection(CurrentFrame,
pKF, sAlreadyFound, th, ORBdist) (ORBmatcher.cc:2325-2447) for one frame table against a batch of candidates equals the Python
restatements of tests/test_reloc_projection_cpu.py exactly (row_point, best_idx and nmatches).  That file shows, on the CPU, that
the constructed scenes take every exit of the reference's loop, match points behind the camera and lose matches to the rotation
filter, so the equalities here are not vacuous."""
import ctypes as C

import numpy as np
import pytest

from pli_slam_amd import capi, realdata, synth
from test_fuse_search_cpu import CAM, IDENTITY, NLEVELS, flip_bits, level_ratio, make_points, make_pose, point_at_pixel, rot_xyz
from test_fuse_search_gpu import real_case
from test_reloc_projection_cpu import (FR, SETTINGS, Cand, behind_case, cand_of, contention_cases, edge_case, filtered_row_case,
                                       frame_of, make_frame, reloc_case, reloc_search_batch, reloc_search_fast, reloc_search_scalar,
                                       reversal_case, wrap360)

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


def frame_kp(fr):
    kp = np.zeros(len(fr.x), capi.KEYPOINT_DT)
    kp["x"], kp["y"], kp["octave"], kp["angle"] = fr.x, fr.y, fr.octave, fr.angle
    kp["size"] = 31.0
    return kp


def call(fe, cands, fr, th=10.0, orb_dist=100, check_ori=True, cam=CAM):
    return fe.search_by_projection_reloc([tuple(cd) for cd in cands], frame_kp(fr), fr.desc, cam, th, orb_dist, check_ori,
                                         level_ratio=level_ratio())


def check(fe, cands, fr, th=10.0, orb_dist=100, check_ori=True, scalar=False, cam=CAM):
    rows, bi, nm = call(fe, cands, fr, th, orb_dist, check_ori, cam)
    assert rows.shape == (len(cands), len(fr.x)) and nm.shape == (len(cands),) and len(bi) == len(cands)
    wr, wi, wn = reloc_search_batch(cands, fr, cam, th, orb_dist, check_ori, reloc_search_scalar if scalar else reloc_search_fast)
    for k in range(len(cands)):
        assert np.array_equal(bi[k], wi[k]), "candidate %d: %d of %d best_idx differ" % (k, int((bi[k] != wi[k]).sum()), len(wi[k]))
        assert np.array_equal(rows[k], wr[k]), "candidate %d: %d row_point differ" % (k, int((rows[k] != wr[k]).sum()))
    assert np.array_equal(nm, wn)
    return rows, bi, nm


@pytest.mark.parametrize("ncand", [0, 1, 3])
def test_constructed_scenes(fe, ncand):
    """400 frame rows against ncand candidates of 400 points each, a tenth of the rows occupied at entry and a tenth of the points
    invalid: the two settings of Tracking.cc:4290 / :4304, with and without the rotation filter; the scalar restatement once per
    setting."""
    fr, cands, _ = reloc_case(np.random.default_rng(500 + ncand), ncand)
    total = filtered = 0
    for th, orb_dist in SETTINGS:
        rows, bi, nm = check(fe, cands, fr, th, orb_dist)
        total += int(nm.sum())
        filtered += sum(int((b >= 0).sum()) for b in bi) - int(nm.sum())
        check(fe, cands, fr, th, orb_dist, check_ori=False)
        if ncand:
            check(fe, cands[:1], fr, th, orb_dist, scalar=True)                          # the reference's control flow
    print("ncand %d: %d matches over the two settings, %d more removed by the rotation filter" % (ncand, total, filtered))
    if ncand:
        assert total > 40 * ncand and filtered > 0
        plain = [cd._replace(occupied=None) for cd in cands]                            # no occupied table
        check(fe, plain, fr, 10.0, 100)
    else:
        assert total == 0


def test_hand_worked_cases(fe):
    for name, (cd, fr, kw, rows, best) in contention_cases().items():
        r, b, n = check(fe, [cd], fr, scalar=True, **kw)
        assert (r[0].tolist(), b[0].tolist()) == (rows, best), name
    cd, fr = behind_case()                                                               # a point behind the camera matches
    assert check(fe, [cd], fr, scalar=True)[0][0].tolist() == [0]
    cd, fr, u = edge_case()                                                              # u == mnMaxX is inside
    assert u == CAM.max_x and check(fe, [cd], fr, scalar=True)[0][0].tolist() == [0]
    pts, descs, fr = reversal_case()                                                     # contention, both list orders
    assert check(fe, [cand_of(pts, descs)], fr)[0][0].tolist() == [0, 1, 2]
    assert check(fe, [cand_of(pts[::-1].copy(), descs[::-1].copy())], fr)[0][0].tolist() == [1, 0, 2]
    cd, fr, rows, best, nm = filtered_row_case()                                         # a filtered row blocked and ends as -1
    r, b, n = check(fe, [cd], fr, scalar=True)
    assert (r[0].tolist(), b[0].tolist(), int(n[0])) == (rows, best, nm)
    r, b, n = check(fe, [cd], fr, check_ori=False, scalar=True)
    assert r[0].tolist() == best and n[0] == 12


def test_thresholds(fe):
    rng = np.random.default_rng(7)
    d = rng.integers(0, 256, 32, dtype=np.uint8)
    P = point_at_pixel(300.0, 200.0)
    for th, orb_dist in SETTINGS:
        for nbits in (orb_dist - 1, orb_dist, orb_dist + 1):
            _, b, n = check(fe, [cand_of(P, [d])], frame_of([300], [200], [flip_bits(rng, d, nbits)]), th, orb_dist, scalar=True)
            assert b[0].tolist() == [0 if nbits <= orb_dist else -1] and n[0] == (nbits <= orb_dist), (orb_dist, nbits)


def crowded_scene(rng, nspots=30, nkeys=10, rep=40, npts=500):
    """Crowded copies (rep keypoints within +-2.5 px of each of nkeys keypoints, the descriptor copied too) and npts points on
    nspots spots.  -> frame, crowded frame, points, descs, pose"""
    spots, sdesc = make_points(rng, nspots)
    spots["valid"] = 1
    pose = make_pose(rot_xyz(0.01, 0.01, -0.01), [0.1, 0.05, -0.1])
    fr, _ = make_frame(rng, spots, sdesc, pose, nkeys)
    x = (np.repeat(fr.x, rep) + rng.uniform(-2.5, 2.5, len(fr.x) * rep)).astype(np.float32)
    y = (np.repeat(fr.y, rep) + rng.uniform(-2.5, 2.5, len(fr.x) * rep)).astype(np.float32)
    crowded = FR(x, y, np.repeat(fr.octave, rep), np.repeat(fr.desc, rep, axis=0), wrap360(rng.uniform(0, 360, len(x))))
    pick = rng.integers(0, nspots, npts)
    return fr, crowded, spots[pick], sdesc[pick], pose


def test_windows_with_more_candidates_than_the_list(fe):
    """Windows of 40 to 100 candidates within ORBdist, above the candidate list's width, so the ordered phase walks those windows
    itself, a dozen points per spot taking one row after the other."""
    rng = np.random.default_rng(8)
    fr, crowded, pts, descs, pose = crowded_scene(rng)
    assert len(crowded.x) == 400
    ang = wrap360(rng.uniform(0, 360, len(pts)))
    cd = Cand(pts, descs, ang, pose, None)
    for th, orb_dist in SETTINGS:
        _, bi, nm = check(fe, [cd], crowded, th, orb_dist, check_ori=False)
        assert nm[0] > 30
        check(fe, [cd, cd._replace(occupied=(rng.random(400) < 0.3).astype(np.uint8))], crowded, th, orb_dist)
    same = crowded._replace(desc=np.zeros_like(crowded.desc))
    zero = cd._replace(descs=np.zeros_like(descs))
    _, bi, nm = check(fe, [zero], same, 10.0, 100, check_ori=False)
    assert nm[0] > 60
    check(fe, [zero._replace(points=pts[:120], descs=zero.descs[:120], angles=ang[:120])], same, 3.0, 64, scalar=True)


def test_the_same_candidate_twice_in_one_batch(fe):
    """Different poses and different occupied rows for the same point list: the candidates do not share owner state."""
    rng = np.random.default_rng(13)
    fr, cands, _ = reloc_case(rng, 1)
    cd = cands[0]
    R = rot_xyz(0.0005, -0.0004, 0.0003) @ cd.pose[:9].reshape(3, 3).astype(np.float64)
    other = cd._replace(pose=make_pose(R, cd.pose[9:12] + np.float32(0.002)), occupied=(rng.random(len(fr.x)) < 0.3).astype(np.uint8))
    batch = [cd, other, cd._replace(occupied=None)]
    rows, bi, nm = check(fe, batch, fr, 10.0, 100)
    for k in range(3):
        r1, b1, n1 = call(fe, batch[k:k + 1], fr, 10.0, 100)
        assert np.array_equal(r1[0], rows[k]) and np.array_equal(b1[0], bi[k]) and n1[0] == nm[k]
    assert nm.min() > 30 and not np.array_equal(bi[0], bi[1]) and not np.array_equal(bi[0], bi[2])
    for _ in range(2):                                                   # calls repeat
        r2, b2, n2 = call(fe, batch, fr, 10.0, 100)
        assert np.array_equal(r2, rows) and np.array_equal(n2, nm) and all(np.array_equal(x, y) for x, y in zip(b2, bi))


def test_real_orb_tables(fe):
    """Tables of the device's own extractor (real_case), cut to 500 points by 400 rows: the points of frame 0 searched for in its
    right image, in the next frame and in itself; the angles are the extractor's where the point has a keypoint."""
    cam = CAM._replace(fx=np.float32(fe.cfg.fx), fy=np.float32(fe.cfg.fx), bf=np.float32(fe.cfg.bf))
    rng = np.random.default_rng(21)
    total = 0
    frames = realdata.frames_752x480(2, seed=4)
    for pair in ([synth.make_stereo_pair(3, W, H, t=0), synth.make_stereo_pair(3, W, H, t=1)], [frames[0], frames[1]]):
        pts, descs, kfs = real_case(fe, pair, cam)
        pts, descs = pts[:500], descs[:500]
        for kf in kfs:
            fr = FR(kf.x[:400], kf.y[:400], kf.octave[:400], kf.desc[:400], wrap360(rng.uniform(0, 30, min(400, len(kf.x)))))
            cands = [Cand(pts, descs, wrap360(rng.uniform(40, 70, len(pts))), kf.pose, (rng.random(len(fr.x)) < 0.1).astype(np.uint8)),
                     Cand(pts[::2], descs[::2], wrap360(rng.uniform(0, 360, len(pts[::2]))), kf.pose, None)]
            for th, orb_dist in SETTINGS:
                total += int(check(fe, cands, fr, th, orb_dist, cam=cam)[2].sum())
    print("real ORB tables: %d matches" % total)
    assert total > 100, total


def test_capacity_arguments_and_empty_sides(fe):
    rng = np.random.default_rng(3)
    cap = 8192                                            # PLI_BOW_MAX_FEATURES
    pts, descs = make_points(rng, 200)
    ang = wrap360(rng.uniform(0, 360, 200))
    cd = Cand(pts, descs, ang, IDENTITY, None)

    def table(n):
        return FR(rng.uniform(0, W, n).astype(np.float32), rng.uniform(0, H, n).astype(np.float32),
                  rng.integers(0, NLEVELS, n).astype(np.int32), rng.integers(0, 256, (n, 32), dtype=np.uint8),
                  wrap360(rng.uniform(0, 360, n)))
    small, big, full, empty = table(50), table(cap + 1), table(cap), table(0)
    with pytest.raises(capi.PliError) as e:
        call(fe, [cd], big)
    assert e.value.status == -3                     # PLI_ERR_CAPACITY: nf = 8193
    occ = (rng.random(cap) < 0.5).astype(np.uint8)
    check(fe, [cd._replace(occupied=occ), cd], full, 10.0, 100)                          # nf exactly at the cap
    for orb_dist in (-1, 256):
        with pytest.raises(capi.PliError) as e:
            call(fe, [cd], small, 10.0, orb_dist)
        assert e.value.status == -1, orb_dist       # PLI_ERR_INVALID
    check(fe, [cd], small, 10.0, 255)               # the largest threshold
    check(fe, [cd], small, 10.0, 0)
    bad = small._replace(octave=np.concatenate([small.octave[:-1], [NLEVELS]]).astype(np.int32))
    with pytest.raises(capi.PliError) as e:
        call(fe, [cd], bad)
    assert e.value.status == -1
    lr = level_ratio().copy()
    lr[3] = lr[1]
    with pytest.raises(capi.PliError) as e:
        fe.search_by_projection_reloc([tuple(cd)], frame_kp(small), small.desc, CAM, level_ratio=lr)
    assert e.value.status == -1
    with pytest.raises(capi.PliError) as e:         # an angle outside [0, 360) with check_orientation
        call(fe, [cd._replace(angles=np.full(200, 360.0, np.float32))], small)
    assert e.value.status == -1
    check(fe, [cd._replace(angles=np.full(200, 360.0, np.float32))], small, check_ori=False)      # not read without it
    # empty sides: a candidate without points inside a batch, nothing but empty lists, no frame rows, no candidates
    none = Cand(pts[:0], descs[:0], ang[:0], IDENTITY, None)
    rows, bi, nm = check(fe, [none, cd, none], small)
    assert (rows[0] == -1).all() and len(bi[0]) == 0 and nm[0] == 0 and nm[2] == 0
    rows, bi, nm = check(fe, [none, none], small)
    assert (rows == -1).all() and (nm == 0).all()
    rows, bi, nm = check(fe, [cd, none], empty)
    assert rows.shape == (2, 0) and (bi[0] == -1).all() and (nm == 0).all()
    rows, bi, nm = call(fe, [], small)
    assert rows.shape == (0, 50) and bi == [] and nm.shape == (0,)
    # raw calls: mp_off decreasing or not starting at 0, every null pointer
    L, h, ptr = fe.L, fe.h, capi.ptr
    kp, kd = frame_kp(small), np.ascontiguousarray(small.desc)
    mp, md = np.ascontiguousarray(pts), np.ascontiguousarray(descs)
    pose = np.stack([IDENTITY, IDENTITY])
    camc = capi.FuseCamera(*[float(v) for v in CAM])
    out, nmo, lvr = np.zeros(100, np.int32), np.zeros(2, np.int32), level_ratio()

    def raw(off, mp=mp, md=md, ma=ang, po=pose, kkp=kp, kkd=kd, cam=camc, lv=lvr, rp=out, nm=nmo, ori=1):
        off = None if off is None else np.array(off, np.int32)
        return L.pli_search_by_projection_reloc(h, 2, ptr(off), ptr(mp), ptr(md), ptr(ma), ptr(po), ptr(kkp), ptr(kkd), 50, None,
                                                C.byref(cam) if cam is not None else None, 10.0, ptr(lv), 100, ori, ptr(rp), None,
                                                ptr(nm))
    assert raw([0, 80, 200]) == 0
    assert raw([0, 80, 200], ma=None, ori=0) == 0                                      # mp_angle may be NULL without the filter
    assert raw([0, 120, 80]) == -1 and raw([1, 80, 200]) == -1
    for kw in (dict(mp=None), dict(md=None), dict(ma=None), dict(po=None), dict(kkp=None), dict(kkd=None), dict(cam=None),
               dict(lv=None), dict(rp=None), dict(nm=None)):
        assert raw([0, 80, 200], **kw) == -1, kw
    assert raw(None) == -1
    assert L.pli_search_by_projection_reloc(None, 2, ptr(np.array([0, 80, 200], np.int32)), ptr(mp), ptr(md), ptr(ang), ptr(pose),
                                            ptr(kp), ptr(kd), 50, None, C.byref(camc), 10.0, ptr(lvr), 100, 1, ptr(out), None,
                                            ptr(nmo)) == -1
