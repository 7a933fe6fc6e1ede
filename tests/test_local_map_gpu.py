"""pli_search_local_points / pli_search_local_lines on the MI355X (the product library) equal, byte for byte, (a) the numpy
restatement of tests/helpers_local_map.py and (b) Frontend.search_local_map / Frontend.match_nnr fed the queries and the list the
host builds.  tests/test_local_map_cpu.py shows on the CPU that the scenes take every exit and that the constructed rows reject
the misreadings, so the equalities are not vacuous.  (A NaN is compared as a NaN: helpers_local_map.canonical.)"""
import ctypes as C

import numpy as np
import pytest

import helpers_local_map as lm
from helpers_local_map import CAM, IDENTITY, f32
from pli_slam_amd import capi
from test_fuse_search_cpu import NLEVELS, level_ratio

pytestmark = pytest.mark.gpu
W, H = 752, 480
BOUNDS = (CAM.min_x, CAM.max_x, CAM.min_y, CAM.max_y)
SEED = 21


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


def check_points(fe, pose, pts, descs, kp, desc, ur, occ, th=1.0, far=False, th_far=0.0):
    view, best, n_in_view, nmatches = fe.search_local_points(pts, descs, pose, CAM, kp, desc, ur, th=th, far_points=far,
                                                             th_far=th_far, cur_occupied=occ, level_ratio=level_ratio())
    wv, wb, wn, wm, q = lm.search_local_points(pts, descs, pose, kp, desc, ur, occ, th=th, far_points=far, th_far=th_far)
    assert lm.canonical(view) == lm.canonical(wv.astype(capi.LOCAL_VIEW_DT)), "%d records differ" % int(
        sum(lm.canonical(view[i:i + 1]) != lm.canonical(wv[i:i + 1]) for i in range(len(wv))))
    assert best.tobytes() == wb.tobytes(), "%d of %d best_idx2 differ" % (int((best != wb).sum()), len(wb))
    assert (n_in_view, nmatches) == (wn, wm)
    # the parent's path: the same queries, built on the host, through pli_search_local_map
    pn, pb = fe.search_local_map(q, descs, kp, desc, ur, BOUNDS, 0.8, occ) if len(q) else (0, np.zeros(0, np.int32))
    assert best.tobytes() == pb.tobytes() and nmatches == pn
    return view, best, n_in_view, nmatches


@pytest.mark.parametrize("nq", [0, 1, 63, 64, 65, 257, 300])
def test_points_against_300_keypoints(fe, nq):
    pose, pts, descs, kp, desc, ur, occ = lm.point_scene(SEED, 300, 300)
    total = 0
    for th, far in ((1.0, False), (3.0, False), (1.0, True), (3.0, True)):
        _, _, nv, nm = check_points(fe, pose, pts[:nq], descs[:nq], kp, desc, ur, occ, th, far, 12.0)
        total += nm
    print("nq %d: %d in view, %d matches over the four settings" % (nq, nv, total))
    if nq >= 257:
        assert nv > 80 and total > 40


def test_points_all_invalid_and_an_empty_frame(fe):
    pose, pts, descs, kp, desc, ur, occ = lm.point_scene(SEED, 300, 300)
    dead = pts.copy()
    dead["valid"] = 0
    view, best, nv, nm = check_points(fe, pose, dead, descs, kp, desc, ur, occ)
    assert nv == 0 and nm == 0 and not np.frombuffer(view.tobytes(), np.uint8).any()
    view, best, nv, nm = check_points(fe, pose, pts, descs, kp[:0], desc[:0], ur[:0], None)
    assert nv > 80 and nm == 0 and (best == -1).all()


def test_points_a_frame_above_the_lds_owner_table_takes_the_scan(fe):
    pose, pts, descs, kp, desc, ur, occ = lm.point_scene(SEED + 1, 50, 15361)
    _, _, nv, nm = check_points(fe, pose, pts, descs, kp, desc, ur, occ, th=3.0)
    print("scan: %d in view, %d matches" % (nv, nm))
    assert nv >= 10 and nm >= 5


def test_points_constructed_rows(fe):
    rows = np.concatenate([lm.point_on_the_far_corner(), lm.one_point((0.0, 0.0, 0.0)), lm.one_point((1.0, 0.0, 0.0)),
                           lm.one_point((-1.0, 0.0, 0.0)), lm.point_where_the_angle_tests_disagree()])
    kp = np.zeros(4, capi.KEYPOINT_DT)
    kp["x"], kp["y"] = (0.0, 100.0, CAM.max_x - 7, CAM.max_x), (0.0, 100.0, CAM.max_y - 6, CAM.max_y)   # (the last: outside the grid)
    kp["octave"] = (NLEVELS - 1, NLEVELS - 1, 0, 0)
    desc = np.zeros((4, 32), np.uint8)
    view, best, nv, nm = check_points(fe, IDENTITY, rows, np.zeros((5, 32), np.uint8), kp, desc, np.full(4, -1, f32), None, th=3.0)
    assert view["in_view"].tolist() == [1, 1, 0, 0, 1] and nv == 3
    assert view["proj_x"][0] == CAM.max_x and view["proj_y"][0] == CAM.max_y and np.isnan(view["proj_x"][1])
    assert view["proj_x"][2] == -1 and view["proj_x"][3] == -1 and view["view_cos"][4] == f32(0.5)
    assert best[0] == 2 and best[1] == -1, best                  # the corner point matches; the NaN query takes no keypoint


def test_points_stored_views_take_part_in_list_order(fe):
    """Points skipped at Tracking.cc:3813 that still have mbTrackInView set: every fifth row of the scene becomes a stored view
    aimed at a keypoint (or at nothing), with and without the far-point gate."""
    pose, pts, descs, kp, desc, ur, occ = lm.point_scene(SEED, 300, 300)
    rng = np.random.default_rng(5)
    pts, descs = pts.copy(), descs.copy()
    plain = check_points(fe, pose, pts, descs, kp, desc, ur, occ, th=3.0)[1]
    for i in range(0, 300, 5):
        j = int(rng.integers(0, 300))
        aimed = rng.random() < 0.7
        x, y = (kp["x"][j] + rng.uniform(-2, 2), kp["y"][j] + rng.uniform(-2, 2)) if aimed else rng.uniform(-50, 800, 2)
        pts[i:i + 1] = lm.stored_view(x, y, x - rng.uniform(1, 30), rng.uniform(1, 20), rng.uniform(0.99, 1.0), int(kp["octave"][j]))
        descs[i] = desc[j]
    assert capi.LOCAL_STORED_VIEW == lm.STORED_VIEW
    stored = pts["valid"] == lm.STORED_VIEW
    view, best, nv, nm = check_points(fe, pose, pts, descs, kp, desc, ur, occ, th=3.0)
    took = int((best[stored] >= 0).sum())
    moved = int((best[~stored] != plain[~stored]).sum())
    print("stored views: %d of %d took a keypoint, %d other points got another answer" % (took, stored.sum(), moved))
    assert took >= 10 and took < stored.sum() and moved >= 3 and not view["in_view"][stored].any()
    check_points(fe, pose, pts, descs, kp, desc, ur, occ, th=1.0, far=True, th_far=12.0)
    # a stored level outside the pyramid is refused before any device call
    pts[0:1] = lm.stored_view(10.0, 10.0, 5.0, 3.0, 0.9, NLEVELS)
    with pytest.raises(capi.PliError):
        fe.search_local_points(pts, descs, pose, CAM, kp, desc, ur, level_ratio=level_ratio())


def check_lines(fe, pose, sp, valid, descs, cur, nnr=0.9):
    in_view, proj, lst, m, n = fe.search_local_lines(sp, valid, descs, pose, CAM, cur, nnr)
    wi, wp, wl, wm, wn = lm.search_local_lines(sp, valid, descs, pose, cur, nnr)
    assert in_view.tobytes() == wi.tobytes() and lm.canonical(proj) == lm.canonical(wp)
    assert lst.tobytes() == wl.tobytes() and m.tobytes() == wm.tobytes() and n == wn
    pn, pm = fe.match_nnr(descs[wl], cur, nnr) if len(wl) else (0, np.zeros(0, np.int32))      # the parent's path
    assert m.tobytes() == pm.tobytes() and n == pn
    return lst, m, n


@pytest.mark.parametrize("nl", [0, 1, 64, 65, 300])
def test_lines(fe, nl):
    pose, sp, valid, descs, cur = lm.line_scene(SEED, 300, 60)
    lst, m, n = check_lines(fe, pose, sp[:nl], valid[:nl], descs[:nl], cur)
    print("nl %d: %d in view, %d matches" % (nl, len(lst), n))
    if nl == 300:
        assert len(lst) > 100 and n > 10


def test_lines_above_one_chunk_of_the_workgroup(fe):
    pose, sp, valid, descs, cur = lm.line_scene(SEED + 2, 2500, 40)
    lst, m, n = check_lines(fe, pose, sp, valid, descs, cur)
    assert len(lst) > 1024 and n > 5


@pytest.mark.parametrize("n2", [0, 1, 2])
def test_lines_few_frame_lines(fe, n2):
    pose, sp, valid, descs, cur = lm.line_scene(SEED, 300, 60)
    lst, m, n = check_lines(fe, pose, sp, valid, descs, cur[:n2])
    assert len(lst) > 100 and (n2 == 2 or (n == 0 and (m == -1).all()))


def test_lines_none_in_view_and_the_constructed_row(fe):
    pose, sp, valid, descs, cur = lm.line_scene(SEED, 300, 60)
    lst, m, n = check_lines(fe, pose, sp, np.zeros(300, np.uint8), descs, cur)
    assert len(lst) == 0 and n == 0
    behind = sp.copy()
    behind[:, 2] = -np.abs(behind[:, 2]) - 30
    lst, _, _ = check_lines(fe, IDENTITY, behind, valid, descs, cur)
    assert len(lst) == 0
    row = lm.line_where_the_two_forms_disagree()
    a, _ = lm.is_in_frustum_l(row, [1], IDENTITY)
    lst, _, _ = check_lines(fe, IDENTITY, row, np.ones(1, np.uint8), descs[:1], cur)
    assert len(lst) == a[0]


def test_negative_counts_with_a_live_context(fe):
    cam = capi.FuseCamera(*[float(v) for v in CAM])
    buf = np.zeros(64, np.uint8)
    lr = level_ratio()
    n1, n2 = C.c_int32(), C.c_int32()
    p = capi.ptr
    assert fe.L.pli_search_local_points(fe.h, p(buf), p(buf), -1, p(IDENTITY), C.byref(cam), 0.5, 1.0, 0, 0.0, 0.8, p(lr), p(buf),
                                        p(buf), p(buf), None, 0, p(buf), p(buf), C.byref(n1), C.byref(n2)) == -1
    assert fe.L.pli_search_local_points(fe.h, p(buf), p(buf), 0, p(IDENTITY), C.byref(cam), 0.5, 1.0, 0, 0.0, 0.8, p(lr), p(buf),
                                        p(buf), p(buf), None, -1, p(buf), p(buf), C.byref(n1), C.byref(n2)) == -1
    assert fe.L.pli_search_local_lines(fe.h, p(buf), p(buf), p(buf), 1, p(IDENTITY), C.byref(cam), p(buf), -1, 0.9, p(buf),
                                       p(buf), p(buf), p(buf), C.byref(n1), C.byref(n2)) == -1
    assert fe.L.pli_search_local_lines(fe.h, p(buf), p(buf), p(buf), -1, p(IDENTITY), C.byref(cam), p(buf), 1, 0.9, p(buf),
                                       p(buf), p(buf), p(buf), C.byref(n1), C.byref(n2)) == -1
