"""KannalaBrandt8 pinned to the reference's own compiled src/CameraModels/KannalaBrandt8.cpp, as float arithmetic, and the
two-camera branches of SearchByProjection(F, vpMapPoints, ...), SearchByProjection(CurrentFrame, LastFrame, ...),
SearchForTriangulation (mpCamera2 on both keyframes), SearchByBoW(pKF, F, ...) (F.Nleft != -1) and Fuse(pKF, vpMapPoints, th, bRight)
pinned to its src/ORBmatcher.cc: the restatements of test_triangulation_two_cameras_cpu.py,
test_bow_two_cameras_cpu.py and test_fuse_two_cameras_cpu.py, scalar and closed form, equal the recorded answers exactly with no row left out; hand cases hold the named edges; every exit is taken five times over
the fixtures; every misreading switch of those files is rejected by a reference fixture; the host arithmetic of the relative and
right poses - the restatements' and the adapter's own, compiled for the host - equals the stand-in's cv::Mat bit for bit.

tests/golden/match_ref_two_cameras holds, per case of tests/helpers_match_ref_two_cameras.py, tables of points, pixels and keypoint
pairs and what oracle/_ref/pli_ref_match (function "kb8": the reference's KannalaBrandt8.cpp compiled where it lies against the
stand-in of oracle/ref_recipe/match_shim; see oracle/Makefile) returned for project, unproject and TriangulateMatches.  Here,
without a device:

  * where the reference program is present it is run again and must reproduce every recorded array, and the generators still build
    the recorded inputs;
  * oracle.kb8_project, oracle.kb8_unproject and the triangulation inside oracle.stereo_fisheye equal the recorded floats bit for
    bit, except at the inputs where the C library's atan2f / tanf (what the compiled reference imports; it imports sincos, sqrtf,
    fminf, fmaxf besides, and no cosf / sinf) returned a float next to the correctly rounded one.  Those inputs are found in float64
    here (helpers: project32 / unproject32 with the libm result moved by one float) and counted; a difference anywhere else fails;
  * helpers_geometry's float64 model agrees with the recorded floats within the envelope that file measures;
  * the corpus holds the named edges: the optical axis, z < 0, x = 0, y = 0, a Newton loop of ten steps and of one, both sides of
    the parallax gate, both depth-sign exits and both reprojection gates.

What the pin covers: KannalaBrandt8.cpp's own scalar arithmetic, gates and the overloads its calls select, over this project's
statement of cv::Mat, cv::SVD::compute and Mat / s (the stand-in says which).  Result: no expression differs; the
residue is glibc's rounding of atan2f and tanf alone.
"""
import os
from collections import Counter

import numpy as np
import pytest

import helpers_geometry as G
import helpers_match_ref_two_cameras as H

ids = lambda c: c.name
f32 = np.float32


def _same_bits(a, b):
    return np.asarray(a, f32).tobytes() == np.asarray(b, f32).tobytes()


def test_corpus_is_the_fixture_directory_and_stays_small():
    assert sorted(os.listdir(H.GOLD_DIR)) == sorted(c.name + ".npz" for c in H.CASES)
    assert sum(os.path.getsize(H.fixture_path(c.name)) for c in H.CASES) <= H.SIZE_CAP
    for c in H.KB8_CASES:
        a, res = H.load_fixture(c.name)
        assert sorted(res) == sorted(c.calls), c.name
        assert 2 * len(a["kp1"]) <= H.MAX_ROWS, c.name                    # the pairs as two tables: features of both cameras together
        assert len(a["points"]) <= H.MAX_POINTS and len(a["pixels"]) <= H.MAX_POINTS, c.name
    for c in H.FUSE2_CASES:
        a, res = H.load_fixture(c.name)
        assert sorted(res) == sorted(c.calls), c.name
        assert len(a["kf_x"]) <= H.MAX_ROWS and int(a["nmp"][0]) <= H.MAX_POINTS, c.name
        assert len(a["kf_x"]) - int(a["kf_nleft"][0]) <= int(a["kf_nleft"][0]), c.name      # mvuRight has Nleft entries (Frame.cc:1589)
    for c in H.LOCAL2_CASES + H.FRAME2_CASES:
        a, res = H.load_fixture(c.name)
        assert sorted(res) == sorted(c.calls), c.name
        assert len(a["cur_x"]) <= H.MAX_ROWS and len(a["mp_bad"]) <= H.MAX_POINTS, c.name            # both cameras' features together
    for c in H.TRI2_CASES + H.BOW2_CASES:
        a, res = H.load_fixture(c.name)
        assert sorted(res) == sorted(c.calls), c.name
        tables = [k for k in a if k.endswith("_node")]
        assert len(tables) <= H.MAX_TABLES and max(len(a[k]) for k in tables) <= H.MAX_ROWS, c.name      # both cameras' features together


@pytest.mark.skipif(not set(H.FUNCTIONS) <= H.ref_functions(),
                    reason="oracle/_ref/pli_ref_match with the two-camera functions is built only where the reference tree exists")
@pytest.mark.parametrize("case", H.CASES, ids=ids)
def test_live_reference_equals_fixture(case):
    """(The program is asked which functions it has: one built from the single-camera recipe, left over where the reference tree
    is gone, cannot run these cases and says so.)"""
    a, results = H.load_fixture(case.name)
    live_inputs = case.arrays()
    assert sorted(live_inputs) == sorted(a), case.name
    for k, v in live_inputs.items():                                      # the generators still build the recorded inputs
        assert np.asarray(v).tobytes() == a[k].tobytes() and np.asarray(v).shape == a[k].shape, (case.name, k)
    for call in case.calls:
        res = H.run_reference(case.bag(a, call))
        assert sorted(res) == sorted(results[call]), (case.name, call)
        for k, v in res.items():
            assert v.dtype == results[call][k].dtype and v.shape == results[call][k].shape and v.tobytes() == results[call][k].tobytes(), (
                case.name, call, k, H.LIBM_HINT if case.fn == "kb8" else "")


@pytest.mark.parametrize("case", H.TRI2_CASES + H.BOW2_CASES + H.FUSE2_CASES, ids=ids)
def test_restatements_equal_the_reference(case):
    """No row is left out: every pair that reaches the triangulation gate is decided with margin (asserted; SearchByBoW is integers
    only), and the whole match container and the return value equal the reference's for every call."""
    a, results = H.load_fixture(case.name)
    if case.fn == "tri2" or (case.fn == "fuse2" and not case.tags):          # (fuse2's hand cases sit ON their thresholds, exactly)
        assert case.undecided(a) == 0
    for call in case.calls:
        want = case.expected(a, call, results[call])
        assert H.same(want, case.restate(a, call)), (case.name, call, "scalar restatement")
        assert H.same(want, case.restate(a, call, fast=True)), (case.name, call, "closed-form restatement")


def test_the_hand_case_is_the_worked_answer():
    """tri2_hand (its docstring works the answers out): all four (bRight1, bRight2) combinations decide a row, the later idx2 wins a
    tie, a distance exactly at TH_LOW matches, the gate alone turns a candidate away, bCoarse skips it, bOnlyStereo returns nothing."""
    case = H.BY_NAME["tri2_hand"]
    a, results = H.load_fixture(case.name)
    for call in case.calls:
        _, (os_, co, ori) = case._call(call)
        m, n = case.expected(a, call, results[call])
        want = [-1, -1, -1, -1] if os_ else [4, 1, 3, 2] if co else [4, 1, 3, 6]
        if ori and not os_:
            want = case.restate(a, call)[0].tolist()                         # (four matches, equal angles: the filter keeps them)
            assert want == ([4, 1, 3, 2] if co else [4, 1, 3, 6])
        assert m.tolist() == want and n == sum(v >= 0 for v in want), (call, m)


def test_host_arithmetic_of_the_poses_equals_the_stand_ins_cv_mat():
    """The four relative poses of ORBmatcher.cc:995-1003 and the right-pose getters of KeyFrame.cc:1343-1373 as the stand-in's cv::Mat
    evaluates them (recorded by the driver beside every tri2 call) against test_triangulation_two_cameras_cpu.relative_poses / Pose,
    which the restatements and the device tests take their poses from: bit for bit."""
    import test_triangulation_two_cameras_cpu as T2
    poses = {"tri2_hand": [T2.POSE_B], "tri2_corpus": [T2.POSE_B, T2.POSE_C, T2.POSE_B]}
    for case in H.TRI2_CASES:
        a, results = H.load_fixture(case.name)
        for call in case.calls:
            k = case._call(call)[0]
            r = results[call]
            assert r["rel"].tobytes() == a["n%d_rel" % k].tobytes() == T2.relative_poses(T2.POSE_A, poses[case.name][k]).tobytes(), (case.name, call)
            for row, p in zip(r["right_poses"], (T2.POSE_A, poses[case.name][k])):
                twr = T2.gemm(p.R.T, T2.TLR_T, 1.0, p.centre())                 # GetRightCameraCenter: Rwl * tlr + twl
                want = np.concatenate([p.right_rotation().reshape(9), p.right_translation().reshape(3), twr.reshape(3)])
                assert row.tobytes() == want.astype(f32).tobytes(), (case.name, call)


@pytest.mark.parametrize("case", H.LOCAL2_CASES, ids=ids)
def test_local_map_restatement_and_oracle_equal_the_reference(oracle, case):
    """SearchByProjection(F, vpMapPoints, ...) with F.Nleft != -1: the Python restatement (Local2Case.restate) and
    oracle.search_local_map_fisheye leave the reference's map point in every one of the frame's Nleft + Nright slots and return its
    count.  The function projects nothing (the track fields are the queries), so no row can be undecided and none is left out."""
    a, results = H.load_fixture(case.name)
    want = case.expected(a, "call", results["call"])
    assert H.same(want, case.restate(a)), (case.name, "restatement")
    assert H.same(want, case.oracle(oracle, a)), (case.name, "oracle")


def test_the_local_map_hand_cases_are_the_worked_answers():
    """local2_hand / local2_hand_ratio07 (the builder's docstring works them out): mbTrackInView only, mbTrackInViewR only, both; a left
    match copied to mvLeftToRightMatch[bestIdx] + Nleft and the mirror; best / second best on one level at the ratio boundary and
    one past it, on each side - and the left failure leaving the right camera unsearched; an observed right slot; TH_HIGH."""
    for name in ("local2_hand", "local2_hand_ratio07"):
        a, results = H.load_fixture(name)
        assert H.same(H.BY_NAME[name].expected(a, "call", results["call"]), H.local2_hand_want(a)), name


def test_every_local_map_exit_is_taken_five_times_on_each_camera():
    total = Counter()
    for case in H.LOCAL2_CASES:
        case.restate(H.load_fixture(case.name)[0], exits=total)
    print("SearchByProjection(F, vpMapPoints), two cameras, exits over the fixtures:", {k: total[k] for k in H.Local2Case.exits})
    for name in H.Local2Case.exits:                                           # (_L / _R: the exit on each camera)
        assert total[name] >= 5, (name, dict(total))


@pytest.mark.parametrize("name", H.Local2Case.misreadings)
def test_a_deliberate_local_map_misreading_is_rejected_by_a_reference_fixture(name):
    caught = []
    for case in H.LOCAL2_CASES:
        a, results = H.load_fixture(case.name)
        if not H.same(case.expected(a, "call", results["call"]), case.restate(a, misread=(name,))):
            caught.append(case.name)
    print("misreading %s: rejected by %s" % (name, caught))
    assert caught, name
    assert name == "th_on_right" or any("hand" in c for c in caught), (name, caught)      # (th != 1 is a seeded scene's)


@pytest.mark.parametrize("case", H.FRAME2_CASES, ids=ids)
def test_frame_to_frame_restatements_equal_the_reference(case):
    """SearchByProjection(CurrentFrame, LastFrame, th, bMono) with CurrentFrame.Nleft != -1: two_camera_scalar and two_camera_fast of
    test_two_camera_projection_cpu.py, on the queries the case's exact projections give, leave the reference's map point in every one
    of the frame's Nleft + Nright slots and return its count.  The projections are exact in float (identity pinhole, z = 1, Trl a
    translation) and everything after them is float comparison without libm: no row can be undecided and none is left out."""
    a, results = H.load_fixture(case.name)
    want = case.expected(a, "call", results["call"])
    assert H.same(want, case.restate(a)), (case.name, "scalar restatement")
    assert H.same(want, case.restate(a, fast=True)), (case.name, "closed-form restatement")


def test_the_frame_to_frame_hand_cases_are_the_worked_answers():
    """frame2_hand* (the builder's docstring): the left image gate and the empty left window leave the right camera unsearched; a left
    search with candidates but no match while the right matches; the right winner at bestIdx2 + Nleft; a right candidate occupied
    through mvpMapPoints[i2 + Nleft]; TH_HIGH on each side; the forward / backward / neutral octave window on the right; a match in
    each half that the joint rotation histogram removes and a one-camera histogram would keep."""
    for case in H.FRAME2_CASES:
        if case.tags:
            a, results = H.load_fixture(case.name)
            assert H.same(case.expected(a, "call", results["call"]), H.frame2_hand_want(a)), case.name


def test_every_frame_to_frame_exit_is_taken_five_times_on_each_camera():
    total = Counter()
    for case in H.FRAME2_CASES:
        case.restate(H.load_fixture(case.name)[0], exits=total)
    print("SearchByProjection(CurrentFrame, LastFrame), two cameras, exits over the fixtures:", dict(sorted(total.items())))
    for name in ("invalid_L", "outside_bounds_L", "window_empty_L", "all_occupied_L", "none_free_L", "all_above_TH_HIGH_L", "distance_above_TH_HIGH_L",
                 "matched_L", "filtered_L", "skipped_R", "window_empty_R", "all_occupied_R", "none_free_R", "all_above_TH_HIGH_R",
                 "distance_above_TH_HIGH_R", "matched_R", "filtered_R"):
        assert total[name] >= 5, (name, dict(total))


@pytest.mark.parametrize("name", H.Frame2Case.misreadings)
def test_a_deliberate_frame_to_frame_misreading_is_rejected_by_a_reference_fixture(name):
    caught = []
    for case in H.FRAME2_CASES:
        a, results = H.load_fixture(case.name)
        if not H.same(case.expected(a, "call", results["call"]), case.restate(a, misread=(name,))):
            caught.append(case.name)
    print("misreading %s: rejected by %s" % (name, caught))
    assert any("hand" in c for c in caught), (name, caught)                   # a hand case, not only the seeded scenes


def test_the_fuse_hand_cases_are_the_worked_answers():
    """fuse2_hand_* (the builder's docstring): a right winner returned as its row + NLeft, the earlier of two equal distances across a
    cell border, a keypoint exactly at the radius, a point with z < 0 that the fisheye model still projects, a candidate rejected
    only by the 5.99 gate, a distance exactly at TH_LOW, a projection exactly on mnMaxX."""
    for which, want in H.FUSE2_HAND.items():
        case = H.BY_NAME["fuse2_hand_" + which]
        a, results = H.load_fixture(case.name)
        for call, rows in zip(case.calls, want):
            best, ops, kf_mp, _, ret = case.expected(a, call, results[call])
            assert best.tolist() == rows and ret == sum(r >= 0 for r in rows), (which, call, best)
            if rows[0] >= 0:                                                  # AddObservation then AddMapPoint on the row found
                assert ops.tolist() == [[4, 0, rows[0]], [5, 0, rows[0]]] and kf_mp[rows[0]] == 0, (which, call, ops)


def test_every_fuse_exit_is_taken_five_times_on_each_camera():
    for call in ("left", "right"):
        total = Counter()
        for case in H.FUSE2_CASES:
            a, _ = H.load_fixture(case.name)
            if call in case.calls:
                case.restate(a, call, exits=total)
        print("Fuse(pKF, vpMapPoints, th, bRight = %d), exits over the fixtures:" % (call == "right"), dict(total))
        for name in H.Fuse2Case.exits:
            assert total[name] >= 5, (call, name, dict(total))


@pytest.mark.parametrize("switch", ["left_pose_for_right", "left_cam_for_right", "left_grid_for_right", "no_nleft", "pinhole", "stereo_bound",
                                    "no_depth_gate"])
def test_a_deliberate_fuse_misreading_is_rejected_by_a_reference_fixture(switch):
    from dataclasses import replace
    import test_fuse_two_cameras_cpu as F2
    rules = replace(F2.REF, **{switch: True})
    caught = []
    for case in H.FUSE2_CASES:
        a, results = H.load_fixture(case.name)
        caught += [case.name + "/" + call for call in case.calls
                   if not H.same(case.expected(a, call, results[call])[0], case.restate(a, call, rules=rules)[0])]
    print("misreading %s: rejected by %s" % (switch, caught))
    assert caught, switch
    if switch != "pinhole":                            # (no hand case tells Pinhole::project from KannalaBrandt8::project off the axis)
        assert any(c.startswith("fuse2_hand_") for c in caught), (switch, caught)


ADAPTER_SRC = r'''
#define PLI_ADAPTER_NO_KEYLINE_HEADER
#define PLI_ADAPTER_KEYLINE_TYPE StubKeyLine
#include <opencv2/core/core.hpp>
struct StubKeyLine { float angle; int class_id; int octave; cv::Point2f pt; float response; float size; float startPointX,
  startPointY, endPointX, endPointY, sPointInOctaveX, sPointInOctaveY, ePointInOctaveX, ePointInOctaveY, lineLength; int numOfPixels; };
#include "pli_slam_amd/adapters/orbslam_two_cameras.hpp"
#include <cstdio>
struct KeyFrame {                          // what the two functions read of a keyframe; the getters as KeyFrame.cc:1343-1373 writes them
  cv::Mat Tcw, Ow, mTlr;
  cv::Mat GetRotation() { return Tcw.rowRange(0, 3).colRange(0, 3).clone(); }
  cv::Mat GetTranslation() { return Tcw.rowRange(0, 3).col(3).clone(); }
  cv::Mat GetCameraCenter() { return Ow.clone(); }
  cv::Mat GetRightCameraCenter() {
    cv::Mat Rwl = Tcw.rowRange(0, 3).colRange(0, 3).t();
    cv::Mat tlr = mTlr.rowRange(0, 3).col(3);
    cv::Mat twl = Ow.clone();
    cv::Mat twr = Rwl * tlr + twl;
    return twr.clone();
  }
  cv::Mat GetRightRotation() {
    cv::Mat Rrl = mTlr.rowRange(0, 3).colRange(0, 3).t();
    cv::Mat Rlw = Tcw.rowRange(0, 3).colRange(0, 3).clone();
    cv::Mat Rrw = Rrl * Rlw;
    return Rrw.clone();
  }
  cv::Mat GetRightTranslation() {
    cv::Mat Rrl = mTlr.rowRange(0, 3).colRange(0, 3).t();
    cv::Mat tlw = Tcw.rowRange(0, 3).col(3).clone();
    cv::Mat trl = -Rrl * mTlr.rowRange(0, 3).col(3);
    cv::Mat trw = Rrl * tlw + trl;
    return trw.clone();
  }
};
static void fill(KeyFrame& K, const float* Tlr, const float* pose) {      // pose: Rcw row major, tcw, Ow
  K.Tcw = cv::Mat::eye(4, 4, CV_32F); K.Ow = cv::Mat(3, 1, CV_32F); K.mTlr = cv::Mat(3, 4, CV_32F);
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) K.Tcw.at<float>(i, j) = pose[3 * i + j];
    K.Tcw.at<float>(i, 3) = pose[9 + i]; K.Ow.at<float>(i) = pose[12 + i];
    for (int j = 0; j < 4; ++j) K.mTlr.at<float>(i, j) = Tlr[4 * i + j];
  }
}
int main(int argc, char** argv) {          // IN: Tlr[12], then pose1[15] pose2[15] per pair; OUT per pair: rel[48], poses of pKF1 [30], of pKF2 [30]
  FILE* in = std::fopen(argv[1], "rb");
  FILE* out = std::fopen(argv[2], "wb");
  float Tlr[12], p[30];
  if (!in || !out || std::fread(Tlr, 4, 12, in) != 12) return 2;
  while (std::fread(p, 4, 30, in) == 30) {
    KeyFrame k1, k2;
    fill(k1, Tlr, p); fill(k2, Tlr, p + 15);
    float res[108];
    ORB_SLAM3::pli_detail::relativePosesTwoCameras(&k1, &k2, res);
    ORB_SLAM3::pli_detail::fusePosesTwoCameras(&k1, res + 48);
    ORB_SLAM3::pli_detail::fusePosesTwoCameras(&k2, res + 78);
    std::fwrite(res, 4, 108, out);
  }
  return std::fclose(out);
}
'''


def test_the_adapters_pose_arithmetic_equals_the_stand_ins_cv_mat(tmp_path):
    '''pli_detail::relativePosesTwoCameras and fusePosesTwoCameras - what PliORBmatcherTwoCameras::SearchForTriangulation and ::Fuse
    hand to the device - compiled for the host: on the poses of the tri2 fixtures (every keyframe pair) and of the fuse2 fixtures
    they give, bit for bit, the four relative poses of ORBmatcher.cc:995-1003 and the right poses of KeyFrame.cc:1343-1373 as the
    stand-in's cv::Mat evaluates them (recorded by the driver beside every tri2 call), and the left poses unchanged.'''
    import subprocess
    src, exe = str(tmp_path / "poses.cpp"), str(tmp_path / "poses")
    open(src, "w").write(ADAPTER_SRC)
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", H.ROOT, "-I", os.path.join(H.ROOT, "tests", "stubs"), "-o", exe, src],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    pairs, want, Tlr = [], [], None
    for case in H.TRI2_CASES:
        a, results = H.load_fixture(case.name)
        Tlr = a["Tlr"]
        for k in range(sum(1 for key in a if key.endswith("_pose2"))):
            res = results["n%d_s000" % k]
            pairs.append(np.concatenate([a["pose1"], a["n%d_pose2" % k]]))
            want.append(np.concatenate([res["rel"].reshape(48), a["pose1"], res["right_poses"][0], a["n%d_pose2" % k], res["right_poses"][1]]))
    with open(tmp_path / "in", "wb") as f:
        f.write(np.asarray(Tlr, f32).tobytes() + np.array(pairs, f32).tobytes())
    subprocess.run([exe, str(tmp_path / "in"), str(tmp_path / "out")], check=True, timeout=60)
    got = np.fromfile(tmp_path / "out", f32).reshape(-1, 108)
    assert len(got) == len(pairs) >= 4
    for g, w in zip(got, want):
        assert g.tobytes() == np.asarray(w, f32).tobytes()
    # Fuse: the keyframes of the fuse2 fixtures carry pose[2, 15] as the restatements and the device tests take it; the adapter's
    # function gives the same 30 floats from the left pose and Tlr
    kfs = [H.load_fixture(c.name)[0] for c in H.FUSE2_CASES]
    with open(tmp_path / "in2", "wb") as f:
        f.write(np.asarray(kfs[0]["Tlr"], f32).tobytes() + np.array([np.concatenate([a["kf_pose"][0], a["kf_pose"][0]]) for a in kfs], f32).tobytes())
    subprocess.run([exe, str(tmp_path / "in2"), str(tmp_path / "out2")], check=True, timeout=60)
    got = np.fromfile(tmp_path / "out2", f32).reshape(-1, 108)
    for g, a in zip(got, kfs):
        assert g[48:78].tobytes() == np.asarray(a["kf_pose"], f32).tobytes()


def test_the_bow_hand_case_is_the_worked_answer():
    """bow2_hand / bow2_hand_filter (the docstring of the builder works the answers out): a right best without a left candidate within
    TH_LOW stays unmatched, a right match is taken where the left failed its ratio test, a right match is taken that a ratio test
    would reject (two equal right distances: the first listed), a left tie fails its ratio test, and the rotation filter removes one
    match of each camera."""
    a, results = H.load_fixture("bow2_hand")
    m, n = H.BY_NAME["bow2_hand"].expected(a, "kf0", results["kf0"])
    assert m.tolist() == H.BOW2_HAND_WANT and n == sum(v >= 0 for v in H.BOW2_HAND_WANT)
    a, results = H.load_fixture("bow2_hand_filter")
    m, n = H.BY_NAME["bow2_hand_filter"].expected(a, "kf0", results["kf0"])
    want = list(H.BOW2_HAND_WANT)
    want[H.BOW2_HAND_NLEFT - 1] = want[-1] = -1                               # the feature turned by 90 degrees, once per camera
    assert m.tolist() == want and n == sum(v >= 0 for v in want)


def test_every_bow_exit_is_taken_five_times_over_the_fixture_corpus():
    total = Counter()
    for case in H.BOW2_CASES:
        a, _ = H.load_fixture(case.name)
        for call in case.calls:
            case.restate(a, call, exits=total)
    print("SearchByBoW(KF, F), two cameras, exits over the fixtures:", dict(total))
    for name in H.Bow2Case.exits:                                             # (the per-camera exits are exits of their own: *_left, *_right)
        assert total[name] >= 5, (name, dict(total))


@pytest.mark.parametrize("switch", ["right_independent", "right_ratio", "right_after_left", "one_top2"])
def test_a_deliberate_bow_misreading_is_rejected_by_a_reference_fixture(switch):
    from dataclasses import replace
    import test_bow_two_cameras_cpu as B2
    rules = replace(B2.REF, **{switch: True})
    caught = []
    for case in H.BOW2_CASES:
        a, results = H.load_fixture(case.name)
        caught += [case.name for call in case.calls if not H.same(case.expected(a, call, results[call]), case.restate(a, call, rules=rules))]
    print("misreading %s: rejected by %s" % (switch, sorted(set(caught))))
    assert caught and any(c.startswith("bow2_hand") for c in caught), switch      # a hand case, not only the seeded scenes


def test_every_exit_is_taken_five_times_over_the_fixture_corpus_on_each_camera():
    from collections import Counter as C
    import test_triangulation_two_cameras_cpu as T2
    total, sides = C(), {0: C(), 1: C()}
    for case in H.TRI2_CASES:
        a, results = H.load_fixture(case.name)
        for call in case.calls:
            ex = C()
            m, _ = case.restate(a, call, exits=ex)
            total.update(ex)
            k = case._call(call)[0]
            t1, nb = case.tables(a, k)
            got = m >= 0
            if call.endswith("_s000"):                                        # each candidate pair once: what the gate said, by kp1's camera
                _, _, gate = case.gate(a, k)
                for i1, i2, _ in T2.candidates(t1, nb.t2):
                    sides[int(i1 >= t1.nleft)]["gate_" + gate.look(i1, i2)[0]] += 1
            sides[0]["matched"] += int(got[:t1.nleft].sum()); sides[1]["matched"] += int(got[t1.nleft:].sum())
            sides[0]["matched_to"] += int((m[got] < nb.t2.nleft).sum()); sides[1]["matched_to"] += int((m[got] >= nb.t2.nleft).sum())
    print("SearchForTriangulation, two cameras, exits over the fixtures:", dict(total), "; by camera:", {k: dict(v) for k, v in sides.items()})
    for name in H.Tri2Case.exits:
        assert total[name] >= 5, (name, dict(total))
    for side in (0, 1):
        assert sides[side]["matched"] >= 5 and sides[side]["matched_to"] >= 5, sides
        for lab in ("ok", "parallax", "z1", "z2", "chi1", "chi2"):            # every exit of the gate on each camera
            assert sides[side]["gate_" + lab] >= 5, (side, lab, dict(sides[side]))


# Deliberate misreadings: the switches of test_triangulation_two_cameras_cpu.TriRules, each rejected by a REFERENCE fixture.
@pytest.mark.parametrize("switch", ["rl_for_lr", "wrong_camera", "swap_sigmas", "first_wins", "epipole_gate"])
def test_a_deliberate_misreading_is_rejected_by_a_reference_fixture(switch):
    from dataclasses import replace
    import test_triangulation_two_cameras_cpu as T2
    rules = replace(T2.REF, **{switch: True})
    caught = []
    for case in H.TRI2_CASES:
        a, results = H.load_fixture(case.name)
        for call in case.calls:
            if call.endswith(("_s000", "_s001")):                              # the gate decides: not bOnlyStereo, not bCoarse
                if not H.same(case.expected(a, call, results[call]), case.restate(a, call, rules=rules)):
                    caught.append(case.name + "/" + call)
    print("misreading %s: rejected by %s" % (switch, caught))
    assert caught, switch
    if switch in ("rl_for_lr", "first_wins"):          # the hand case is built for these two; the other three need a gate near its
        assert any(c.startswith("tri2_hand/") for c in caught), (switch, caught)      # threshold or the epipole: the corpus holds them


def test_the_corpus_holds_the_named_edges():
    labels, steps, axis = Counter(), Counter(), 0
    for c in H.KB8_CASES:
        a, res = H.load_fixture(c.name)
        P = a["points"]
        assert (P[:, 2] < 0).sum() >= 20 and ((P[:, 0] == 0) & (P[:, 1] != 0)).sum() >= 3 and ((P[:, 1] == 0) & (P[:, 0] != 0)).sum() >= 3
        assert ((P[:, 0] == 0) & (P[:, 1] == 0)).sum() >= 3, c.name           # on the optical axis, in front and behind
        for e, cam in ((1, a["cam1"]), (2, a["cam2"])):
            for px in a["pixels"]:
                _, theta, n = H.unproject32(cam, px)
                steps[n] += 1
                axis += theta is None
        lab = [l for l, _, _ in c.labels(a)]
        labels.update(lab)
        want_pos = np.array([l == "ok" for l in lab])                        # every gate decides as the float64 model decides
        assert np.array_equal(res["call"]["tri_ret"] > f32(0.0001), want_pos), c.name
        assert np.all(res["call"]["tri_ret"][[l not in ("ok", "depth_floor") for l in lab]] == f32(-1)), c.name
    print("TriangulateMatches exits over the corpus:", dict(labels), "; Newton steps per unprojected pixel:", dict(sorted(steps.items())))
    assert axis >= 5                                                         # theta_d <= 1e-8: the loop is not entered
    assert steps[10] >= 20 and steps[1] >= 100
    for name in ("ok", "parallax", "z1", "z2", "chi1", "chi2", "depth_floor"):
        assert labels[name] >= 5, (name, dict(labels))


@pytest.mark.parametrize("case", H.KB8_CASES, ids=ids)
def test_oracle_project_and_unproject_equal_the_reference_bit_for_bit(oracle, case):
    """Bit equality, except where the recorded pixel / ray is the one an atan2f / tanf one float off the correctly rounded value
    gives; the oracle then holds the correctly rounded one.  Nothing else may differ."""
    a, res = H.load_fixture(case.name)
    r = res["call"]
    residue = Counter()
    for e, cam in ((1, a["cam1"]), (2, a["cam2"])):
        for p, want in zip(a["points"], r["proj%d" % e]):
            got = oracle.kb8_project(cam, p)
            if _same_bits(got, want):
                continue
            d = H.explain_project(cam, p, want)
            assert d is not None and d != (0, 0), (case.name, e, p, want, got, d)
            assert _same_bits(got, H.project32(cam, p)[0]), (case.name, e, p, got)
            residue["atan2f"] += 1
        for px, want in zip(a["pixels"], r["unproj%d" % e]):
            got = oracle.kb8_unproject(cam, px[0], px[1])
            if _same_bits(got, want):
                continue
            d = H.explain_unproject(cam, px, want)
            assert d is not None and d != 0, (case.name, e, px, want, got, d)
            assert _same_bits(got, H.unproject32(cam, px)[0]), (case.name, e, px, got)
            residue["tanf"] += 1
    n = 2 * (len(a["points"]) + len(a["pixels"]))
    print("%s: %d of %d outputs at an input where glibc's float function is one float off: %s" % (case.name, sum(residue.values()), n, dict(residue)))


def _tolerance(a, case, z):
    tn = float(np.linalg.norm(a["t12"].astype(np.float64)))
    return G.FISHEYE_TOL_C[case.tol] * G.EPS32 * np.maximum(1.0, z * z / tn)


@pytest.mark.parametrize("case", H.KB8_CASES, ids=ids)
def test_oracle_triangulation_equals_the_reference_bit_for_bit(oracle, case):
    """The pairs as two tables whose row i can only match row i, through oracle.stereo_fisheye: depth and p3d equal the recorded
    TriangulateMatches outputs bit for bit.  A pair one of whose two rays the reference computed with a tanf one float off
    (H.tri_residue) is accepted or rejected alike and lies within twice the float64 envelope; no other pair may differ."""
    a, res = H.load_fixture(case.name)
    kpL, dL, kpR, dR = case.tables(a)
    n, l2r, r2l, depth, p3d = oracle.stereo_fisheye(kpL, dL, 0, kpR, dR, 0, a["cam1"], a["cam2"], a["R12"], a["t12"], G.fisheye_sigma2())
    want_depth, want_p3d = H.tri_expected(res["call"])
    residue = H.tri_residue(a, res["call"])
    ok = want_depth > 0
    assert n == int(ok.sum()) and np.array_equal(depth > 0, ok), case.name
    assert np.array_equal(l2r, np.where(ok, np.arange(len(ok)), -1)) and np.array_equal(r2l, l2r), case.name
    differs = (depth.view(np.uint32) != want_depth.view(np.uint32)) | (p3d.view(np.uint32) != want_p3d.view(np.uint32)).any(1)
    assert not np.any(differs & ~residue), (case.name, np.nonzero(differs & ~residue)[0])
    tol = 2 * _tolerance(a, case, want_depth.astype(np.float64))
    assert np.all(np.abs(depth.astype(np.float64) - want_depth) <= tol), case.name
    assert np.all(np.abs(p3d.astype(np.float64) - want_p3d) <= tol[:, None]), case.name
    print("%s: %d of %d pairs at a tanf residue input, %d of them differ" % (case.name, residue.sum(), len(ok), differs.sum()))


def test_float64_model_agrees_with_the_recorded_floats_within_its_envelope():
    """helpers_geometry (float64, shaped differently on purpose) against what the reference computed in float32: the triangulated
    point within FISHEYE_TOL_C units of 2^-23 max(1, z^2 / |t12|), the projections within FISHEYE_MARGIN["px"] at the radius that
    file measured (up to 256 px from the principal point) and in proportion beyond it.  The rays are not compared: the float64 model
    iterates Newton to convergence, and past the clamp at pi / 2 the reference's ten steps converge to nothing."""
    worst = {"depth": 0.0, "p3d": 0.0, "px": 0.0}
    for c in H.KB8_CASES:
        a, res = H.load_fixture(c.name)
        r = res["call"]
        for i, (lab, _, X) in enumerate(c.labels(a)):
            if lab != "ok":
                continue
            tol = _tolerance(a, c, float(X[2]))
            worst["depth"] = max(worst["depth"], abs(float(r["tri_ret"][i]) - X[2]) / tol)
            worst["p3d"] = max(worst["p3d"], float(np.abs(r["tri_p3d"][i].astype(np.float64) - X).max()) / tol)
        for e, cam in ((1, a["cam1"]), (2, a["cam2"])):
            for p, uv in zip(a["points"], r["proj%d" % e]):
                m = G.kb8_project64(cam, p.astype(np.float64))
                radius = max(abs(m[0] - float(cam[2])), abs(m[1] - float(cam[3])))
                worst["px"] = max(worst["px"], float(np.abs(uv.astype(np.float64) - m).max()) / (G.FISHEYE_MARGIN["px"] * max(1.0, radius / 256.0)))
    print("worst observed / allowed: depth %.3f, p3d %.3f, projection %.3f" % (worst["depth"], worst["p3d"], worst["px"]))
    assert worst["depth"] <= 1.0 and worst["p3d"] <= 1.0 and worst["px"] <= 1.0, worst
