"""pli_create_new_map_points on the MI355X (the product library): LocalMapping::CreateNewMapPoints from the search on
(LocalMapping.cc:423-684, keyframes of one pinhole camera) for one keyframe against a batch of neighbours equals the scalar float32
restatement of the reference's SEQUENTIAL loop (tests/helpers_new_map_points.py create_new_map_points) exactly: matches12, nmatches,
status, nnew and the bits of x3d where a map point is created.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import helpers_new_map_points as H
from pli_slam_amd import capi

pytestmark = pytest.mark.gpu
W, Hh = 752, 480
CAMERA = tuple(float(v) for v in H.CAM) + (0.0, float(W), 0.0, float(Hh))


@pytest.fixture(scope="module")
def fe():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from pli_slam_amd.frontend import Frontend
    f = Frontend(capi.default_config(W, Hh), dev=False)
    yield f
    f.close()


def keypoints(t):
    kp = np.zeros(len(t.node), capi.KEYPOINT_DT)
    kp["x"], kp["y"], kp["octave"], kp["angle"] = t.x, t.y, t.octave, t.angle
    kp["size"] = 31.0
    return kp


def kf_of(kf):
    return keypoints(kf.t), kf.t.desc, kf.t.node, kf.t.has_mp, kf.uright, kf.depth, kf.key, kf.pose


def nb_of(nb):
    return kf_of(nb.kf) + (nb.F12, nb.ep)


def cut(kf, rows):
    rows = np.asarray(rows, np.int64)
    return H.KF(type(kf.t)(*[col[rows] for col in kf.t]), kf.uright[rows], kf.depth[rows], kf.key[rows], kf.pose)


def run(fe, kf1, nbrs, coarse=False, far=False, th_far=0.0, cam=H.CAM, mb=H.MB):
    camera = tuple(float(v) for v in cam) + (0.0, float(W), 0.0, float(Hh))
    return fe.create_new_map_points(kf_of(kf1), [nb_of(nb) for nb in nbrs], camera, float(mb), float(H.RATIO_FACTOR), coarse, far,
                                    th_far)


def same(got, want, what=""):
    m, n, s, x, nn = got
    wm, wn, ws, wx, wnn = want
    assert m.shape == wm.shape and s.shape == ws.shape and x.shape == wx.shape
    assert np.array_equal(m, wm), (what, "matches12", np.argwhere(m != wm)[:5])
    assert np.array_equal(n, wn), (what, "nmatches", n, wn)
    bad = np.argwhere(s != ws)
    assert len(bad) == 0, (what, "status", [(tuple(b), H.STATUS[s[tuple(b)]], H.STATUS[ws[tuple(b)]]) for b in bad[:5]])
    assert np.array_equal(nn, wnn), (what, "nnew", nn, wnn)
    made = s == H.CREATED
    assert np.array_equal(x[made].view(np.uint32), wx[made].view(np.uint32)), (what, "x3d bits")


def check(fe, kf1, nbrs, coarse=False, far=False, th_far=0.0, what="", cam=H.CAM, mb=H.MB):
    got = run(fe, kf1, nbrs, coarse, far, th_far, cam, mb)
    same(got, H.create_new_map_points(kf1, nbrs, cam=cam, mb=mb, coarse=coarse, far=far, th_far=th_far), what)
    return got


def test_the_generators_corpus_takes_every_exit_on_the_device(fe):
    """The corpus of tests/test_new_map_points_cpu.py - the seeded scenes of H.SEEDS, on which every exit but w == 0 and dist == 0
    is taken and no pair lies within 2 float ulps of the libm-dependent stereo-parallax comparison, and the two constructed scenes
    that take those two - through the device: equal to the restatement, and every status code comes back from the device."""
    seen = set()
    for seed in H.SEEDS:
        kf1, nbrs = H.scene(seed, 6, 300)
        for coarse, far in ((False, False), (True, True)):
            seen |= set(np.unique(check(fe, kf1, nbrs, coarse, far, 9.0, (seed, coarse, far))[2]).tolist())
    assert seen == set(range(len(H.STATUS))) - {H.CODE["w_zero"], H.CODE["dist_zero"]}
    for c in H.constructed_scenes():
        m, n, s, x, nn = check(fe, c["kf1"], c["nbrs"], what=c["name"], cam=c["cam"], mb=c["mb"])
        assert n.tolist() == [1] and nn.tolist() == [0] and s.tolist() == [[H.CODE[c["name"]]]], (c["name"], n, s)
        seen |= set(s.ravel().tolist())
    assert seen == set(range(len(H.STATUS)))


@pytest.mark.parametrize("nkf", [0, 1, 5, 20])
def test_the_device_equals_the_sequential_loop(fe, nkf):
    """About 300 points; bCoarse and mbFarPoints both ways; from four neighbours on, neighbour 3 has F12 = 0."""
    kf1, nbrs = H.scene(100 + nkf, nkf, 300)
    created = 0
    for coarse, far in ((False, False), (True, True)) if nkf == 20 else ((False, False), (False, True), (True, False), (True, True)):
        got = check(fe, kf1, nbrs, coarse, far, 9.0, (nkf, coarse, far))
        assert got[0].shape == (nkf, len(kf1.t.node))
        created += int(got[4].sum())
        if nkf >= 5:                    # the coupling is exercised: features matched at entry, taken by an earlier neighbour
            assert (got[2] == H.TAKEN_EARLIER).sum() > 0 and (got[4] > 0).sum() >= 3
    assert created > 0 or nkf == 0


@pytest.mark.parametrize("stereo", ["mono", "stereo", "mixed"])
def test_mono_only_stereo_only_and_mixed_tables(fe, stereo):
    kf1, nbrs = H.scene(31, 4, 300, stereo=stereo)
    assert {"mono": (kf1.uright < 0).all(), "stereo": (kf1.uright >= 0).mean() > 0.9, "mixed": True}[stereo]
    for coarse in (False, True):
        got = check(fe, kf1, nbrs, coarse, True, 10.0, (stereo, coarse))
        assert got[4].sum() > 0


def test_neighbours_of_different_sizes_and_empty_ones(fe):
    kf1, nbrs = H.scene(10, 3, 300)
    part = lambda nb, n: nb._replace(kf=cut(nb.kf, np.arange(n)), truth=None)
    mixed = [nbrs[0], part(nbrs[1], 0), part(nbrs[2], 37), part(nbrs[0], 1), nbrs[1]]
    got = check(fe, kf1, mixed)
    assert got[1][1] == 0 and (got[0][1] == -1).all() and (got[2][1] == H.NOT_MATCHED).all()
    # an empty pKF1, and no neighbours
    m, n, s, x, nn = check(fe, cut(kf1, []), mixed)
    assert m.shape == (5, 0) and x.shape == (5, 0, 3) and (n == 0).all() and (nn == 0).all()
    m, n, s, x, nn = run(fe, kf1, [])
    assert m.shape == (0, len(kf1.t.node)) and n.shape == (0,) and nn.shape == (0,)


def test_more_matched_pairs_than_a_workgroup_and_a_single_pair(fe):
    """The compaction crosses waves and blocks (k_newpt_list: 256 pairs a block, one atomic per wave); and a list of one."""
    kf1, nbrs = H.scene(7, 3, 1200, nnodes=40)
    got = check(fe, kf1, nbrs)
    on_entry = (got[0] >= 0) | (got[2] == H.TAKEN_EARLIER)
    assert on_entry.sum() > 1024, on_entry.sum()
    i = int(np.nonzero(got[2][0] == H.CREATED)[0][0])
    one = check(fe, cut(kf1, [i]), nbrs[:1])
    assert one[1].tolist() == [1] and one[4].tolist() == [1] and one[0][0, 0] == got[0][0, i]
    assert np.array_equal(one[3][0, 0].view(np.uint32), got[3][0, i].view(np.uint32))


def test_a_batch_equals_single_calls_chained_by_hand_and_calls_repeat(fe):
    kf1, nbrs = H.scene(9, 7, 300, nnodes=20)
    for coarse in (False, True):
        batch = run(fe, kf1, nbrs, coarse, True, 9.0)
        has = kf1.t.has_mp.copy()
        for k, nb in enumerate(nbrs):                        # the reference's loop, one call per neighbour
            m, n, s, x, nn = run(fe, kf1._replace(t=kf1.t._replace(has_mp=has)), [nb], coarse, True, 9.0)
            assert np.array_equal(m[0], batch[0][k]) and n[0] == batch[1][k] and nn[0] == batch[4][k]
            made = s[0] == H.CREATED
            assert np.array_equal(made, batch[2][k] == H.CREATED)
            assert np.array_equal(x[0][made].view(np.uint32), batch[3][k][made].view(np.uint32))
            seen = batch[2][k] != H.TAKEN_EARLIER            # (a single call cannot tell "taken earlier" from "has a map point")
            assert np.array_equal(s[0][seen], batch[2][k][seen]) and (s[0][~seen] == H.NOT_MATCHED).all()
            has[made] = 1
        for _ in range(3):
            again = run(fe, kf1, nbrs, coarse, True, 9.0)
            assert all(np.array_equal(a, b) for a, b in zip(again, batch))
        assert batch[4].sum() > 0


def test_capacity_and_arguments(fe):
    cap = 8192                                            # PLI_BOW_MAX_FEATURES
    kf1, nbrs = H.scene(3, 2, 60)
    grow = lambda kf, n: cut(kf, np.arange(n) % len(kf.t.node))
    big = grow(kf1, cap + 1)
    for a, b in ((big, nbrs), (kf1, [nbrs[0], nbrs[1]._replace(kf=grow(nbrs[1].kf, cap + 1))])):
        with pytest.raises(capi.PliError) as e:
            run(fe, a, b)
        assert e.value.status == -3                 # PLI_ERR_CAPACITY
    # exactly at the cap, on either side
    check(fe, grow(kf1, cap), nbrs[:1], coarse=True)
    check(fe, kf1, [nbrs[0]._replace(kf=grow(nbrs[0].kf, cap))], coarse=True)

    def spoil(kf, field, value):
        if field in ("octave", "x", "node"):
            col = getattr(kf.t, field).copy()
            col[-1] = value
            return kf._replace(t=kf.t._replace(**{field: col}))
        col = getattr(kf, field).copy()
        col.reshape(-1)[-1] = value
        return kf._replace(**{field: col})
    for field, value in (("octave", 8), ("octave", -1), ("node", -2), ("x", np.nan), ("uright", np.inf), ("depth", np.nan),
                         ("key", np.inf), ("pose", np.nan)):
        for a, b in ((spoil(kf1, field, value), nbrs), (kf1, [nbrs[0], nbrs[1]._replace(kf=spoil(nbrs[1].kf, field, value))])):
            with pytest.raises(capi.PliError) as e:
                run(fe, a, b)
            assert e.value.status == -1, (field, value)            # PLI_ERR_INVALID
    # a decreasing kf_off, a negative count and null tables, at the C ABI
    p = capi.ptr
    k1, d1, n1, m1, u1, z1, p1, pose1 = [np.ascontiguousarray(a) for a in kf_of(kf1)]
    n = len(n1)
    cam = capi.FuseCamera(*CAMERA)
    off = np.array([0, 5, 3], np.int32)
    out_i, out_f, cnt = np.zeros((2, n), np.int32), np.zeros((2, n, 3), np.float32), np.zeros(2, np.int32)
    f12, ep, pose = np.zeros((2, 9), np.float32), np.zeros((2, 2), np.float32), np.zeros((2, 15), np.float32)

    def call(n1_, nkf, off_, kk):
        return fe.L.pli_create_new_map_points(fe.h, p(k1), p(d1), p(n1), p(m1), p(u1), p(z1), p(p1), n1_, nkf, p(off_), kk, p(d1), p(n1),
                                              p(m1), p(u1), p(z1), p(p1), p(f12), p(ep), p(pose1), p(pose), C.byref(cam), 0.1, 0, 0, 0.0,
                                              1.8, p(out_i), p(cnt), p(out_i), p(out_f), p(cnt))
    assert call(n, 2, off, p(k1)) == -1
    assert call(-1, 2, np.array([0, 1, 2], np.int32), p(k1)) == -1
    assert call(n, -1, np.array([0, 1, 2], np.int32), p(k1)) == -1
    assert call(n, 2, np.array([0, 1, 2], np.int32), None) == -1
    assert call(n, 2, np.array([0, 0, 0], np.int32), None) == 0          # empty neighbours need no tables
