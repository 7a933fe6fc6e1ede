"""The restatement of Frame::isInFrustum / isInFrustum_l and of the local-map queries (tests/helpers_local_map.py) on the CPU: the
seeded scenes take every exit, the constructed rows reject the misreadings they were built against, and a plain float64
evaluation agrees wherever a gate has a margin."""
import math
from collections import Counter

import numpy as np

import helpers_local_map as lm
from helpers_local_map import CAM, IDENTITY, f32, f64
from test_fuse_search_cpu import NLEVELS

SEED, NQ, NCUR = 21, 900, 300
TH_FAR = 12.0


def test_the_point_scene_takes_every_exit():
    pose, pts, descs, kp, desc, ur, occ = lm.point_scene(SEED, NQ, NCUR)
    exits = Counter()
    view, best, n_in_view, nmatches, q = lm.search_local_points(pts, descs, pose, kp, desc, ur, occ, far_points=True, th_far=TH_FAR,
                                                               exits=exits)
    print("exits", dict(exits), "in view", n_in_view, "matches", nmatches)
    for name in lm.POINT_EXITS:
        assert exits[name] >= 5, (name, exits)
    assert sum(exits.values()) == NQ and exits["in_view"] == n_in_view
    seen = view[view["in_view"] == 1]
    levels = Counter(seen["level"].tolist())
    print("levels", dict(levels))
    assert all(levels[l] >= 3 for l in range(NLEVELS)), levels
    wide, narrow = int((seen["view_cos"].astype(f64) <= 0.998).sum()), int((seen["view_cos"].astype(f64) > 0.998).sum())
    far = int((seen["depth"] > f32(TH_FAR)).sum())
    print("view_cos <= 0.998:", wide, "> 0.998:", narrow, "far points:", far)
    assert wide >= 10 and narrow >= 10 and far >= 10
    assert int(q["valid"].sum()) == n_in_view - far
    # a point refused after the image gate keeps its projection, one refused before it keeps -1
    late = (view["in_view"] == 0) & (view["proj_x"] != -1) & (pts["valid"] != 0)
    assert late.sum() == exits["too_near"] + exits["too_far"] + exits["view_angle"]
    assert nmatches >= 30 and (best >= 0).sum() == nmatches
    # th != 1 multiplies the radius; far points off lets the far points search
    q3 = lm.local_queries(view, th=3.0)
    assert int(q3["valid"].sum()) == n_in_view
    r = np.where(seen["view_cos"].astype(f64) > 0.998, f32(2.5), f32(4.0))
    assert np.array_equal(q3["radius"][view["in_view"] == 1], ((r * f32(3.0)).astype(f32) * lm.SF[seen["level"]]).astype(f32))


def test_the_line_scene_takes_every_exit_and_keeps_list_order():
    pose, sp, valid, descs, cur = lm.line_scene(SEED, 400, 60)
    exits = Counter()
    in_view, proj, lst, m, n = lm.search_local_lines(sp, valid, descs, pose, cur, 0.9, exits=exits)
    print("exits", dict(exits), "matches", n)
    for name in lm.LINE_EXITS:
        assert exits[name] >= 5, (name, exits)
    assert np.all(np.diff(lst) > 0) and len(lst) == exits["in_view"] == int(in_view.sum())
    assert n >= 10 and len(m) == len(lst)
    assert np.all(proj[in_view == 0] == 0)


def test_constructed_far_corner_is_in_view_here_and_out_under_IsInImage():
    P = lm.point_on_the_far_corner()
    V = lm.is_in_frustum(P, IDENTITY)[0]
    assert V["in_view"] == 1 and V["proj_x"] == CAM.max_x and V["proj_y"] == CAM.max_y
    W = lm.is_in_frustum(P, IDENTITY, misread=("image_half_open",))[0]
    assert W["in_view"] == 0 and W["proj_x"] == -1


def test_constructed_depth_zero_nan_stays_and_infinity_leaves():
    nan_point = lm.one_point((0.0, 0.0, 0.0))
    ex = Counter()
    V = lm.is_in_frustum(nan_point, IDENTITY, exits=ex)[0]
    assert V["in_view"] == 1 and math.isnan(V["proj_x"]) and math.isnan(V["proj_y"]) and V["level"] == NLEVELS - 1, V
    assert lm.is_in_frustum(nan_point, IDENTITY, misread=("nan_out",))[0]["in_view"] == 0
    # ... and takes no keypoint, although one lies wherever a NaN window might be put
    kp = np.zeros(3, lm.hm.KEYPOINT_DT); kp["octave"] = NLEVELS - 1
    kp["x"], kp["y"] = (0.0, 100.0, CAM.max_x), (0.0, 100.0, CAM.max_y)
    d = np.zeros((3, 32), np.uint8)
    _, best, n_in_view, nmatches, q = lm.search_local_points(nan_point, d[:1], IDENTITY, kp, d, np.full(3, -1, f32), None)
    assert n_in_view == 1 and np.isnan(q["u"][0]) and q["valid"][0] == 0 and nmatches == 0 and best[0] == -1
    # +inf and -inf are refused at the image gate (not at the depth gate: 0.0f < 0.0f is false) and leave -1 behind
    for x, exit_ in ((1.0, "right"), (-1.0, "left")):
        ex = Counter()
        V = lm.is_in_frustum(lm.one_point((x, 0.0, 0.0)), IDENTITY, exits=ex)[0]
        assert ex[exit_] == 1 and V["in_view"] == 0 and V["proj_x"] == -1 and V["proj_y"] == -1, (x, ex, V)


def test_constructed_viewing_angle_float_and_double_disagree():
    P = lm.point_where_the_angle_tests_disagree()
    assert lm.is_in_frustum(P, IDENTITY)[0]["in_view"] == 1
    assert lm.is_in_frustum(P, IDENTITY)[0]["view_cos"] == f32(0.5)
    assert lm.is_in_frustum(P, IDENTITY, misread=("normal_double",))[0]["in_view"] == 0


def test_constructed_line_the_two_projection_forms_differ_across_the_bound():
    sp = lm.line_where_the_two_forms_disagree()
    a, _ = lm.is_in_frustum_l(sp, [1], IDENTITY)
    b, _ = lm.is_in_frustum_l(sp, [1], IDENTITY, misread=("pinhole_form",))
    assert a[0] != b[0]
    # the same coordinates as a point go the other way: isInFrustum divides
    P = lm.one_point(sp[0])
    assert lm.is_in_frustum(P, IDENTITY)[0]["proj_x"] != lm.is_in_frustum(P, IDENTITY, misread=("invz_form",))[0]["proj_x"]


def test_a_stored_view_is_searched_in_its_list_position_with_the_fields_it_holds():
    """A point that Tracking.cc:3813 skips keeps mbTrackInView from an earlier frame (one camera: :2996-3004 resets only
    mbTrackInViewR) and ORBmatcher.cc:53 searches it: it takes a keypoint, and so changes what the points behind it get."""
    kp = np.zeros(2, lm.hm.KEYPOINT_DT)
    kp["x"], kp["y"], kp["octave"] = (300.0, 500.0), (200.0, 300.0), (2, 2)
    desc = np.zeros((2, 32), np.uint8)
    ur = np.full(2, -1, f32)
    live = lm.one_point(((300.0 - float(CAM.cx)) * 4 / float(CAM.fx), (200.0 - float(CAM.cy)) * 4 / float(CAM.fy), 4.0),
                        normal=(0.0, 0.0, 1.0), max_dist=4.0 * 1.2 ** 1.5)
    V = lm.is_in_frustum(live, IDENTITY)[0]
    assert V["in_view"] == 1 and V["level"] == 2 and abs(V["proj_x"] - 300) < 1e-3
    stale = lm.stored_view(301.0, 201.0, 290.0, 5.0, 0.9, 2)
    far_stale = lm.stored_view(301.0, 201.0, 290.0, 50.0, 0.9, 2)
    empty = lm.stored_view(100.0, 100.0, 90.0, 5.0, 0.9, 2)
    d = np.zeros((2, 32), np.uint8)
    # alone, the live point takes keypoint 0; behind a stored view it finds the row taken
    assert lm.search_local_points(live, d[:1], IDENTITY, kp, desc, ur, None)[1].tolist() == [0]
    view, best, n_in_view, nmatches, q = lm.search_local_points(np.concatenate([stale, live]), d, IDENTITY, kp, desc, ur, None)
    assert best.tolist() == [0, -1] and n_in_view == 1 and nmatches == 1 and q["valid"].tolist() == [1, 1]
    assert not np.frombuffer(view[:1].tobytes(), np.uint8).any()              # its record is not this call's
    assert lm.search_local_points(np.concatenate([live, stale]), d, IDENTITY, kp, desc, ur, None)[1].tolist() == [0, -1]
    # no keypoint in the stored window; the far-point gate reads the stored depth
    assert lm.search_local_points(np.concatenate([empty, live]), d, IDENTITY, kp, desc, ur, None)[1].tolist() == [-1, 0]
    assert lm.search_local_points(np.concatenate([far_stale, live]), d, IDENTITY, kp, desc, ur, None, far_points=True,
                                  th_far=12.0)[1].tolist() == [-1, 0]


def test_float64_evaluation_of_the_lines_agrees_wherever_a_gate_has_a_margin():
    """The same comparison for isInFrustum_l: fx*X*invz + cx is three roundings of values below 1024 (ulp 6.1e-5), so the decisions
    must agree wherever the float64 margin exceeds 1e-3 px, and the projections to that bound."""
    pose, sp, valid, _, _ = lm.line_scene(SEED, 400, 60)
    in_view, proj = lm.is_in_frustum_l(sp, valid, pose)
    R, t = pose[:9].reshape(3, 3).astype(f64), pose[9:12].astype(f64)
    pc = sp.astype(f64) @ R.T + t
    u = float(CAM.fx) * pc[:, 0] / pc[:, 2] + float(CAM.cx)
    v = float(CAM.fy) * pc[:, 1] / pc[:, 2] + float(CAM.cy)
    m_img = np.minimum.reduce([u - float(CAM.min_x), float(CAM.max_x) - u, v - float(CAM.min_y), float(CAM.max_y) - v])
    expect = (valid != 0) & (pc[:, 2] >= 0) & (m_img >= 0)
    clear = (np.abs(pc[:, 2]) > 1e-4) & (np.abs(m_img) > 1e-3)
    print("lines, smallest margins: depth %.3g, image %.3g px; %d of %d rows clear" % (
        np.abs(pc[:, 2]).min(), np.abs(m_img).min(), clear.sum(), len(sp)))
    assert clear.sum() > 0.98 * len(sp)
    assert np.array_equal(in_view[clear] == 1, expect[clear])
    on = in_view == 1
    assert np.abs(proj[on, 0] - u[on]).max() < 1e-3 and np.abs(proj[on, 1] - v[on]).max() < 1e-3


def test_float64_evaluation_agrees_wherever_a_gate_has_a_margin():
    """A plain float64 evaluation of the same geometry.  The float path's projection is a handful of roundings of values below
    1024 (ulp 6.1e-5), its distances and cosine a few relative roundings of 6e-8: the decisions must agree wherever the float64
    margin exceeds 1e-3 px, 1e-5 relative in distance and 1e-5 in cosine, and the values must agree to those bounds."""
    pose, pts, *_ = lm.point_scene(SEED, NQ, NCUR)
    view = lm.is_in_frustum(pts, pose)
    R, t, Ow = pose[:9].reshape(3, 3).astype(f64), pose[9:12].astype(f64), pose[12:15].astype(f64)
    pw = pts["pos"].astype(f64)
    pc = pw @ R.T + t
    with np.errstate(all="ignore"):
        u = float(CAM.fx) * pc[:, 0] / pc[:, 2] + float(CAM.cx)
        v = float(CAM.fy) * pc[:, 1] / pc[:, 2] + float(CAM.cy)
    po = pw - Ow
    dist = np.linalg.norm(po, axis=1)
    cos = (po * pts["normal"].astype(f64)).sum(1) / dist
    m_img = np.minimum.reduce([u - float(CAM.min_x), float(CAM.max_x) - u, v - float(CAM.min_y), float(CAM.max_y) - v])
    m_rng = np.minimum(dist - pts["min_dist_inv"], pts["max_dist_inv"] - dist) / dist
    m_cos = cos - 0.5
    expect = (pts["valid"] != 0) & (pc[:, 2] >= 0) & (m_img >= 0) & (m_rng >= 0) & (m_cos >= 0)
    clear = (np.abs(pc[:, 2]) > 1e-4) & (np.abs(m_img) > 1e-3) & (np.abs(m_rng) > 1e-5) & (np.abs(m_cos) > 1e-5)
    print("smallest margins: depth %.3g, image %.3g px, range %.3g, cosine %.3g; %d of %d rows clear" % (
        np.abs(pc[:, 2]).min(), np.abs(m_img).min(), np.abs(m_rng).min(), np.abs(m_cos).min(), clear.sum(), len(pts)))
    assert clear.sum() > 0.98 * len(pts)
    assert np.array_equal(view["in_view"][clear] == 1, expect[clear])
    on = view["in_view"] == 1
    assert np.abs(view["proj_x"][on] - u[on]).max() < 1e-3 and np.abs(view["proj_y"][on] - v[on]).max() < 1e-3
    assert np.abs(view["view_cos"][on] - cos[on]).max() < 1e-5
    assert np.abs(view["depth"][on] / np.linalg.norm(pc[on], axis=1) - 1).max() < 1e-5
    assert np.abs(view["proj_xr"][on] - (u[on] - float(CAM.bf) / pc[on, 2])).max() < 1e-3
