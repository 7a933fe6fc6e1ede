"""The local-map step, CreateNewMapPoints and ComputeDistinctiveDescriptors pinned to the reference's own compiled code:
Frame::isInFrustum (one camera), Frame::isInFrustum_l, MapPoint::PredictScale(dist, Frame*), Get{Min,Max}DistanceInvariance,
LocalMapping::CreateNewMapPoints (one pinhole camera, and the mpCamera2 branch for two KannalaBrandt8 cameras) with ComputeF12 and
KeyFrame::UnprojectStereo, and MapPoint / MapLine::ComputeDistinctiveDescriptors.

tests/golden/map_ref holds, per case of tests/helpers_map_ref.py, the input tables and what oracle/_ref/pli_ref_map returned (those
definitions cut out of the reference's Frame.cc, MapPoint.cc, MapLine.cc, LocalMapping.cc and KeyFrame.cc at build time and
compiled unmodified, with its whole ORBmatcher.cc and Pinhole.cpp, against the stand-in of oracle/ref_recipe/map_shim; see
oracle/Makefile).  Here, without a device:

  * the restatements (helpers_local_map.is_in_frustum / is_in_frustum_l with the searches behind them, helpers_new_map_points.
    create_new_map_points and closed_form, helpers_distinctive.restated_point / restated_line / independent) equal the recorded
    outputs exactly, and so does the oracle where it has the function (the grid-cell search on the queries of the recorded views);
  * where the reference program is present it is run again and must reproduce every recorded array;
  * every deliberate misreading (the `misread` names of helpers_local_map, helpers_new_map_points.MUTANTS,
    helpers_distinctive.MUTANTS) is rejected by a fixture;
  * the corpus holds the shapes and edges it was built for.

Findings: none that changes an answer the device gives for a defined input.  MapPoint::PredictScale compiles to logf and a float
division (helpers_map_ref.predict_scale_ref): ratio == 1.2f is level 1, where test_fuse_search_cpu.predict_scale (double) says 2; the
C++ adapters compile the reference's expression, case points_level_bounds and the misreading "level_log_double" hold it.  One
input has no defined answer: a point AT the camera centre with mfMaxDistance > 0 has dist 0, and MapPoint.cc:474 converts ceil(log(inf) / mfLogScaleFactor) to int, which C++ leaves
undefined (the x86-64 build that wrote the fixtures returns level 0; this project's PredictScale answers the top level).  The point's
projection is NaN, so its query is closed and the level reaches nothing; case points_infinite_ratio records it and
helpers_map_ref.PointsCase.undefined_level leaves that one field of that one row out.  In the two-camera branch every decision is
held exactly; x3D is held to helpers_new_map_points_two_cameras.MEASURED["x3d_rel"], because KannalaBrandt8::unproject goes through the
C library and about one pixel in thirty unprojects one float away from the oracle's (TwoCamerasCase.same says it in full).
"""
import os

import numpy as np
import pytest

import helpers_distinctive as HD
import helpers_local_map as lm
import helpers_map_ref as H
import helpers_new_map_points as NP
from test_fuse_search_cpu import NLEVELS

ids = lambda c: c.name


def test_corpus_is_the_fixture_directory_and_stays_small():
    assert sorted(os.listdir(H.GOLD_DIR)) == sorted(c.name + ".npz" for c in H.CASES)
    assert sum(os.path.getsize(H.fixture_path(c.name)) for c in H.CASES) <= 1 << 20
    assert set(H.BY_FN) == {c.group or c.fn for c in H.CASES} and all(H.BY_FN.values())


@pytest.mark.parametrize("case", H.CASES, ids=ids)
def test_restatements_equal_the_reference(case):
    a, res = H.load_fixture(case.name)
    want = case.expected(a, res)
    assert case.same(want, case.restate(a)), case.name
    if case.fn == "distinctive":
        for fn in (HD.restated_point, HD.restated_line, HD.independent):
            assert case.same(want, case.restate(a, fn=fn)), (case.name, fn.__name__)
    if case.fn == "new_map_points":
        # closed_form: every pair on the state at entry, first accepted neighbour wins; its creation sequence is the enumeration
        # "neighbours in order, idx1 ascending, status == CREATED" that PliCreateNewMapPoints replays
        assert case.same(want, case.restate(a, closed=True)), (case.name, "closed form")


@pytest.mark.parametrize("case", H.BY_FN["frustum_points"], ids=ids)
def test_oracle_equals_the_reference(oracle, case):
    """oracle/match_oracle.hpp has the grid-cell search over a query table, not isInFrustum: it is fed the queries of
    ORBmatcher.cc:53-73 built from the fields the REFERENCE left in the points, and must leave the rows the reference left."""
    a, res = H.load_fixture(case.name)
    view, best, _, nmatches = case.expected(a, res)
    pts, descs = H.point_rows(a)
    nn, th, far, th_far = a["params"]
    q = lm.local_queries(view, th, bool(far), th_far, points=pts)
    if len(q) == 0:
        return
    n, got = oracle.search_local_map(q, descs, case.kp(a), a["cur_desc"], a["cur_uright"], (a["cur_occ"] == 1).astype(np.uint8),
                                     tuple(float(v) for v in a["cam"][5:9]), float(nn))
    assert got.tobytes() == best.tobytes() and n == nmatches, case.name


@pytest.mark.skipif(not os.path.exists(H.REF_EXE), reason="oracle/_ref/pli_ref_map is built only where the reference tree exists")
@pytest.mark.parametrize("case", H.CASES, ids=ids)
def test_live_reference_equals_fixture(case):
    a, results = H.load_fixture(case.name)
    live_inputs = case.arrays()
    assert sorted(live_inputs) == sorted(a), case.name
    for k, v in live_inputs.items():                                  # the generators still build the recorded inputs
        assert np.asarray(v).tobytes() == a[k].tobytes() and np.asarray(v).shape == a[k].shape, (case.name, k)
    res = H.run_reference(case.bag(a))
    assert sorted(res) == sorted(results), case.name
    for k, v in res.items():
        assert v.dtype == results[k].dtype and v.shape == results[k].shape and v.tobytes() == results[k].tobytes(), (case.name, k)


# Deliberate misreadings, each a parameter of the restatement (its docstring says what it does)
MISREADINGS = {
    "frustum_points": ("image_half_open", "nan_out", "normal_double", "invz_form", "level_log_double"),
    "frustum_lines": ("image_half_open", "nan_out", "pinhole_form"),
    "distinctive": HD.MUTANTS,
    "new_map_points": NP.MUTANTS,
    "new_map_points_two_cameras": ("left_pose_for_right", "left_cam_for_right", "swap_rr_ll"),      # helpers_new_map_points_two_cameras._pick
}


def _rejects(case, name):
    a, res = H.load_fixture(case.name)
    want = case.expected(a, res)
    if case.fn == "new_map_points":                                    # ("last_wins" is the closed form's; the others go to both)
        return not case.same(want, case.restate(a, mut=(name,), closed=True)) and (
            name == "last_wins" or not case.same(want, case.restate(a, mut=(name,))))
    got = case.restate(a, mut=(name,)) if case.fn == "distinctive" else case.restate(a, misread=(name,))
    return not case.same(want, got)


@pytest.mark.parametrize("fn,name", [(fn, m) for fn, ms in MISREADINGS.items() for m in ms], ids=lambda v: v)
def test_a_deliberate_misreading_is_rejected(fn, name):
    small_first = sorted(H.BY_FN[fn], key=lambda c: os.path.getsize(H.fixture_path(c.name)))
    assert any(_rejects(c, name) for c in small_first), (fn, name, "no fixture tells this misreading from the reference")
    if fn == "distinctive":                                            # for points and for lines
        for lines in (False, True):
            assert any(_rejects(c, name) for c in small_first if c.lines(H.load_fixture(c.name)[0]) == lines), (name, lines)


def test_the_misreadings_cover_every_name_of_the_restatements():
    doc = lm.__doc__
    named = {w.strip('"') for w in doc.split() if w.startswith('"') and w.endswith('"')}
    assert named | {"level_log_double"} == set(MISREADINGS["frustum_points"]) | set(MISREADINGS["frustum_lines"]), named
    assert set(MISREADINGS["distinctive"]) == {"median_half", "pick_le"}
    # both stereo parallaxes computed, mvKeysUn in UnprojectStereo, > at the far gate, the neighbour's mbf at :641, last accepted wins
    assert set(MISREADINGS["new_map_points"]) == {"stereo2_always", "unproject_un", "far_gt", "bf_neighbour", "last_wins"}


def test_the_point_corpus_holds_its_shapes_and_edges():
    sizes = sorted(len(H.load_fixture(c.name)[0]["mp_bad"]) for c in H.BY_FN["frustum_points"])
    assert {0, 1, 63, 64, 65, 257} <= set(sizes)
    assert all(len(H.load_fixture(c.name)[0]["cur_x"]) == 300 for c in H.BY_FN["frustum_points"] if c.name.startswith("points_nq"))
    exits = H.exit_counts()["frustum_points"]
    for name in lm.POINT_EXITS + ("stored_view",):
        assert exits[name] >= 5, (name, dict(exits))
    c = H.BY_NAME["points_constructed"]
    a, res = H.load_fixture(c.name)
    view, best, nv, nm = c.expected(a, res)
    cam = H.HM.cam_of(a["cam"])
    # one point on each bound and one on the far corner, all in view; the NaN projection in view, without a keypoint
    assert view["proj_x"][0] == cam.min_x and view["proj_x"][1] == cam.max_x and view["proj_y"][2] == cam.min_y and view["proj_y"][3] == cam.max_y
    assert (view["proj_x"][4], view["proj_y"][4]) == (cam.max_x, cam.max_y) and view["in_view"][:6].tolist() == [1] * 6
    assert np.isnan(view["proj_x"][5]) and np.isnan(view["proj_y"][5]) and best[5] == -1 and best[4] == 2
    # +inf and -inf leave at the image gate, the slightly negative depth at the depth gate: all three keep -1
    assert view["in_view"][6:9].tolist() == [0, 0, 0] and (view["proj_x"][6:9] == -1).all() and a["mp_pos"][8, 2] < 0
    assert view["in_view"][9] == 1 and view["view_cos"][9] == np.float32(0.5)
    # dist equal to 0.8f * mfMinDistance and to 1.2f * mfMaxDistance: both stay
    pts, _ = H.point_rows(a)
    for i, name in ((10, "min_dist_inv"), (11, "max_dist_inv")):
        assert lm._norm3(pts["pos"][i]) == pts[name][i] and view["in_view"][i] == 1, (i, name)
    # the scenes: view_cos on both sides of 0.998, far points behind the gate, every level
    a, res = H.load_fixture("points_nq257")
    view = H.BY_NAME["points_nq257"].expected(a, res)[0]
    seen = view[view["in_view"] == 1]
    assert (seen["view_cos"].astype(np.float64) > 0.998).sum() >= 10 and (seen["view_cos"].astype(np.float64) <= 0.998).sum() >= 10
    assert a["params"][2] == 1 and (seen["depth"] > np.float32(a["params"][3])).sum() >= 10
    assert set(seen["level"].tolist()) == set(range(NLEVELS))
    took = 0
    for name in ("points_stored_views", "points_stored_views_far"):
        a, res = H.load_fixture(name)
        pts, _ = H.point_rows(a)
        stored = pts["valid"] == lm.STORED_VIEW
        best = H.BY_NAME[name].expected(a, res)[1]
        assert stored[::5].all() and not stored[1::5].any(), name                          # interleaved in list order
        took += int((best[stored] >= 0).sum())
        if a["params"][2]:                                                                # the far gate reads the stored depth
            behind = stored & (pts["normal"][:, 0] > np.float32(a["params"][3]))
            assert behind.sum() >= 3 and (best[behind] == -1).all() and (best[stored] >= 0).any(), name
    assert took >= 10, took


def test_the_undefined_level_is_one_field_of_a_closed_query():
    c = H.BY_NAME["points_infinite_ratio"]
    a, res = H.load_fixture(c.name)
    want, got = c.expected(a, res), c.restate(a)
    assert c.undefined_level == (0,) and c.same(want, got)
    assert np.isnan(want[0]["proj_x"][0]) and want[1][0] == -1 and got[0]["level"][0] == NLEVELS - 1
    assert [c2.name for c2 in H.CASES if getattr(c2, "undefined_level", ())] == [c.name]


def test_the_line_corpus_holds_its_shapes_and_edges():
    assert {0, 1, 64, 65, 300} <= {len(H.load_fixture(c.name)[0]["ml_bad"]) for c in H.BY_FN["frustum_lines"]}
    exits = H.exit_counts()["frustum_lines"]
    for name in lm.LINE_EXITS:
        assert exits[name] >= 5, (name, dict(exits))
    a, res = H.load_fixture("lines_none_in_view")
    assert len(res["list"]) == 0 and res["n_to_match"][0] == 0 and len(a["ml_bad"]) == 65
    a, res = H.load_fixture("lines_constructed")
    cam = H.HM.cam_of(a["cam"])
    p = res["proj_s"]
    assert p[0, 0] == cam.min_x and p[1, 0] == cam.max_x and p[2, 1] == cam.min_y and p[3, 1] == cam.max_y and tuple(p[4]) == (cam.max_x, cam.max_y)
    assert res["in_view"][:5].tolist() == [1] * 5 and res["list"].tolist() == np.flatnonzero(res["in_view"]).tolist()
    assert np.isnan(p[7]).all() and res["in_view"][7] == 1                                 # PcZ == 0 with PcX == 0: the NaN stays


def test_the_distinctive_corpus_holds_its_shapes_and_edges():
    for lines in (0, 1):
        name = "distinctive_%s_sizes" % ("lines" if lines else "points")
        a, res = H.load_fixture(name)
        groups = H.groups_of(a)
        sizes = [-1 if g is None else len(g) for g in groups]
        assert {1, 2, 3, 4, 64, 65, 257, 0, -1} <= set(sizes), sizes
        assert a["kf_bad"].sum() == 2 and a["params"][0] == lines
        inside = [f for f in range(len(groups)) if any(a["kf_bad"][k] for ff, k, r in a["obs"] if ff == f)]
        assert len(inside) >= 5                                                            # bad keyframes inside groups
        for f, g in enumerate(groups):
            written = g is not None and len(g) > 0
            assert res["written"][f] == written and (res["row"][f] >= 0) == written, (name, f)
            assert g is None or len({r.tobytes() for r in g}) == len(g)
        assert (res["row"] > 0).sum() >= 3                                                 # winners other than row 0
        a, res = H.load_fixture("distinctive_%s_hand" % ("lines" if lines else "points"))
        ties = 0
        for g in H.groups_of(a):
            b, m, med = HD.independent(g)
            ties += med.count(m) > 1
        assert ties >= 10, ties


def test_the_new_point_corpus_holds_its_shapes_and_edges():
    from collections import Counter
    shapes, f64_exits, restated_exits, coarse = set(), Counter(), Counter(), set()
    for c in H.BY_FN["new_map_points"]:
        a, res = H.load_fixture(c.name)
        extra = H.load_fixture(c.name, "f64")[1]
        kf1, nbrs, cam, mb, bf2, kw = c.scene(a)
        shapes.add((len(nbrs), len(kf1.t.node) >= 250))
        coarse.add(kw["coarse"])
        m, made, x, order = c.expected(a, res)
        # a pair of vMatchedIndices without a created point is rejected: the restatement's exit for it is only held to be no CREATED,
        # and the float64 statement's exit is recorded beside it
        rejected = [(k, i) for k, i, j in res["pairs"] if not made[k, i]]
        assert len(extra["rejected_exit"]) == len(rejected)
        f64_exits.update(NP.STATUS[e] for e in extra["rejected_exit"])
        st = NP.create_new_map_points(kf1, nbrs, cam=cam, mb=mb, bf2=bf2, exits=restated_exits, **kw)[2]
        assert all(st[k, i] != NP.CREATED for k, i in rejected) and ((st == NP.CREATED) == made).all()
        # the one gate a libm decides: no pair within 2 float ulps, judged by the float64 statement (the generator's seeds)
        assert extra["libm_margin_ulps"][0] >= 2.0, (c.name, extra["libm_margin_ulps"])
        # the descriptor a created point is left with: pli_distinctive_descriptors' answer for the two rows in pointer order, row 0
        # (the median index of N = 2 is 0: the diagonal), the CURRENT keyframe's row
        assert (res["desc_row"] == 0).all() and np.array_equal(res["desc"], a["k0_desc"][res["created"][:, 1]]), c.name
        assert all(HD.independent(np.stack([a["k0_desc"][i], a["k%d_desc" % (k + 1)][j]]))[0] == 0 for k, i, j in res["created"][:20])
    print("exits the float64 statement gives the rejected pairs:", dict(f64_exits))
    print("exits of the float32 restatement over the corpus:", dict(restated_exits))
    assert {(1, True), (5, True)} <= shapes and coarse == {False, True}
    for name in ("low_parallax", "empty_unproject", "z1", "z2", "reproj1_mono", "reproj1_stereo", "reproj2_mono", "reproj2_stereo", "far",
                 "ratio_low", "ratio_high"):
        assert f64_exits[name] >= 4 and restated_exits[name] >= 4, (name, f64_exits, restated_exits)
    assert restated_exits["w_zero"] == 1 and restated_exits["taken_earlier"] >= 50
    # more matched pairs at one neighbour than a workgroup has lanes
    a, res = H.load_fixture("newpts_nkf5_mixed_coarse_far")
    assert np.bincount(res["pairs"][:, 0]).max() > 128 and len(res["pairs"]) > 256
    # first accepted wins: a feature accepted at entry by two neighbours, and one matched and rejected in k and accepted in k + 1
    c = H.BY_NAME["newpts_nkf5_mixed_coarse_far"]
    kf1, nbrs, cam, mb, bf2, kw = c.scene(a)
    entry = NP.closed_form(kf1, nbrs, cam=cam, mb=mb, mut=("last_wins",), **kw)[2]         # (the last wins there: what lost is visible)
    first = NP.closed_form(kf1, nbrs, cam=cam, mb=mb, **kw)[2]
    twice = ((entry == NP.CREATED) | (first == NP.CREATED)).sum(0) >= 2
    m, made, _, _ = c.expected(a, res)
    later = [(k, i) for k in range(len(nbrs) - 1) for i in range(m.shape[1]) if m[k, i] >= 0 and not made[k, i] and made[k + 1, i]]
    print("features accepted by two neighbours: %d; rejected in k and accepted in k + 1: %d" % (twice.sum(), len(later)))
    assert twice.sum() >= 5 and len(later) >= 3
    # both sides stereo with the second parallax the smaller one (the else-if), mvKeys != mvKeysUn on an UnprojectStereo row,
    # mvDepth <= 0, dist equal to mThFarPoints
    a, res = H.load_fixture("newpts_nkf2_stereo")
    c = H.BY_NAME["newpts_nkf2_stereo"]
    kf1, nbrs, cam, mb, bf2, kw = c.scene(a)
    smaller = unprojected = 0
    for k, i, j in res["pairs"]:
        S1, S2 = NP.side(kf1, i), NP.side(nbrs[k].kf, j)
        q = {}
        NP.new_map_point_pair(S1, S2, cam, mb, q=q)
        if S1["ur"] >= 0 and S2["ur"] >= 0 and S2["depth"] > 0 and S1["depth"] > 0 and S2["depth"] < S1["depth"]:
            smaller += 1
        if q.get("branch") in ("stereo1", "stereo2"):
            S = S1 if q["branch"] == "stereo1" else S2
            unprojected += int(S["key"][0] != S["x"] or S["key"][1] != S["y"])
    assert smaller >= 10 and unprojected >= 5, (smaller, unprojected)
    assert any((a["k%d_depth" % k][a["k%d_uright" % k] >= 0] <= 0).any() for k in range(3))
    a, res = H.load_fixture("newpts_nkf3_far_on_a_dist")
    c = H.BY_NAME["newpts_nkf3_far_on_a_dist"]
    kf1, nbrs, cam, mb, bf2, kw = c.scene(a)
    on = 0
    for k, i, j in res["pairs"]:
        q = {}
        st, _ = NP.new_map_point_pair(NP.side(kf1, i), NP.side(nbrs[k].kf, j), cam, mb, True, kw["th_far"], q=q)
        on += int(st == NP.CODE["far"] and np.float32(kw["th_far"]) in (np.float32(q["dist1"]), np.float32(q["dist2"])))
    assert on >= 1 and kw["far"]


def test_the_two_camera_corpus_holds_its_shapes_and_edges():
    import helpers_new_map_points_two_cameras as N2
    from collections import Counter
    nkfs, f64_exits = set(), Counter()
    for c in H.BY_FN["new_map_points_two_cameras"]:
        a, res = H.load_fixture(c.name)
        extra = H.load_fixture(c.name, "f64")[1]
        kf1, nbrs, kw = c.scene(a)
        nkfs.add(len(nbrs))
        want = c.expected(a, res)
        got = c.restate(a)
        same, of = c.bit_equal(want, got)
        print("%s: %d of %d created points have the reference's x3D bit for bit; least libm margin %.1f float ulps" % (
            c.name, same, of, extra["libm_margin_ulps"][0]))
        assert same >= 0.9 * of > 0                                      # (the others: one libm result of the unprojection, one float)
        # no pair within 2 float ulps of a comparison that hangs on the KannalaBrandt8 functions, judged by the float64 statement
        assert extra["libm_margin_ulps"][0] >= 2.0, (c.name, extra["libm_margin_ulps"])
        made = want[1]
        rejected = [(k, i) for k, i, j in res["pairs"] if not made[k, i]]
        assert len(extra["rejected_exit"]) == len(rejected)
        f64_exits.update(NP.STATUS[e] for e in extra["rejected_exit"])
        assert all(NP.STATUS[e] in N2.REACHABLE and e != NP.CREATED for e in extra["rejected_exit"])
        # all four (bRight1, bRight2) sides among the points created from ONE neighbour
        sides = Counter((int(i >= kf1.t.nleft), int(j >= nbrs[k].kf.t.nleft)) for k, i, j in res["created"] if k == 0)
        assert set(sides) == {(0, 0), (0, 1), (1, 0), (1, 1)} and min(sides.values()) >= 10, (c.name, sides)
        assert (res["desc_row"] == 0).all() and np.array_equal(res["desc"], a["k0_desc"][res["created"][:, 1]]), c.name
    print("exits the float64 statement gives the rejected pairs:", dict(f64_exits))
    assert nkfs == {1, 3}
    for name in ("low_parallax", "z1", "reproj1_mono", "far", "ratio_low", "ratio_high"):
        assert f64_exits[name] >= 5, (name, f64_exits)
