"""The stereo matchers, LineMatcher and Frame::GetFeaturesInArea held to the reference's own compiled text (CPU only; the device side
is test_ref_pin_stereo_gpu.py).

tests/golden/stereo_ref/ holds what oracle/_ref/pli_ref_stereo returned for every case of tests/helpers_stereo_ref.py: the reference's
src/LineMatcher.cpp as a whole translation unit, its gridStructure.cpp, LineIterator.cpp and Config.cpp, and the stereo functions of
its Frame.cc, compiled against the stand-in of oracle/ref_recipe/stereo_shim.  Here the restatement of tests/helpers_matchers.py and
the oracle (oracle/match_oracle.hpp through pyoracle) must equal those recorded results exactly: floats as bits, mvle_l as double bits,
no tolerance anywhere (the only libm call in these functions is sqrt, which is correctly rounded).

Mutants: every switch of helpers_matchers.Rules, one at a time, must make the restatement differ from at least one reference
fixture.  Three switches cannot be rejected by any table, and the reason is arithmetic, not a hole in the corpus (UNREJECTABLE):
  * ul_minus_001_float: `uL - 0.01` in float or in double is the same float for every uL >= 4.5, which the left window requires
    (tests/test_independent_matchers.py: test_ul_minus_001_in_float_or_in_double_is_the_same_float proves it over the floats);
  * sort_ties_insertion: vDistIdx is filled in iL order, so sorting pairs (ties by iL) and sorting by distance alone (ties in
    insertion order) give one sequence; and the cut keeps exactly the rows whose distance is below thDist, whatever the order;
  * nan_minmax = "fmin" (IEEE fmin / fmax for std::min / std::max): the two differ only where an operand is NaN.  In
    lineSegmentOverlapStereo a NaN left row takes the horizontal branch before any min; a NaN right row makes the projected
    segment (NaN, NaN) under std::min / std::max with a NaN first operand, (x, x) otherwise and under fmin: the overlap is 0 every
    time (NaN length, or an empty intersection).  In filterLineSegmentDisparity min / max of (NaN, x) is NaN / NaN or x / x: the ratio
    is NaN or 1 (or NaN again for x = 0 or inf), never below the threshold.  The NaN rows of the `overlap` and `filter` tables are
    there all the same, and the switch is shown to change nothing on them.
"""
import json
import os
from dataclasses import fields, replace

import numpy as np
import pytest

import helpers_matchers as hm
import helpers_stereo_ref as S

NAMES = S.fixture_names()
POINTS = [n for n in NAMES if n.startswith("points_")]
LINES = [n for n in NAMES if n.startswith("lines_")]
NNR = [n for n in NAMES if n.startswith("nnr_")]
MATCH = [n for n in NAMES if n.startswith("match_")]
DIST = [n for n in NAMES if n.startswith("dist_")]
AREA = [n for n in NAMES if n.startswith("area_")]


@pytest.fixture(scope="module")
def po():
    from oracle import pyoracle
    pyoracle.lib()
    return pyoracle


_CASES = {}


def case(po, name):
    if name not in _CASES:
        _CASES[name] = S.case_of_fixture(name, po.Config, po)
    return _CASES[name]


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def test_fixture_directory_is_complete_and_small():
    assert len(POINTS) >= 20 and len(LINES) >= 15 and len(NNR) >= 30 and len(MATCH) >= 18 and len(DIST) == 2 and len(AREA) == 3
    assert {"images", "descriptor_tables", "overlap", "filter", "rgbd"} <= set(NAMES)
    total = sum(os.path.getsize(os.path.join(S.GOLD_DIR, f)) for f in os.listdir(S.GOLD_DIR))
    assert total <= (1 << 20), total


# ---------------------------------------------------------------------------------------------------------- the two stereo stages
@pytest.mark.parametrize("name", POINTS)
def test_stereo_points_equal_the_reference(po, name):
    c, ref = case(po, name)
    ur, dp = hm.run_points(c)[:2]
    our, odp, _, _ = po.stereo_points_tables(c["cfg"], c["kpL"], c["descL"], c["kpR"], c["descR"], c["pyr"][0], c["pyr"][1])
    for who, a, b in (("restatement", ur, dp), ("oracle", our, odp)):
        for what, got, want in (("mvuRight", a, ref["uright"]), ("mvDepth", b, ref["depth"])):
            assert got.dtype == want.dtype == np.float32
            bad = np.flatnonzero(got.view(np.int32) != want.view(np.int32))
            assert bad.size == 0, "%s: %s of the %s differs from the reference at left keypoints %s" % (name, what, who, bad[:5])


@pytest.mark.parametrize("name", LINES)
def test_stereo_lines_equal_the_reference(po, name):
    c, ref = case(po, name)
    args = (c["cfg"], c["klL"], c["ldL"], c["klR"], c["ldR"], c["W"], c["H"])
    assert ref["disp"].dtype == np.float32 and ref["le"].dtype == np.float64 and ref["m12"].dtype == np.int32
    for who, (disp, le, m12) in (("restatement", hm.stereo_lines(*args)[:3]), ("oracle", po.stereo_lines_tables(*args))):
        for what, got, want in (("mvDisparity_l", disp, ref["disp"]), ("mvle_l", le, ref["le"]), ("matches_12", m12, ref["m12"])):
            assert got.dtype == want.dtype and bits(got) == bits(want), "%s: %s of the %s differs from the reference at left lines %s" % (
                name, what, who, np.flatnonzero((got.reshape(len(got), -1) != want.reshape(len(want), -1)).any(1))[:5])


def test_overlap_and_filter_tables_equal_the_reference():
    ins, ref = S.load_fixture("overlap")
    got = np.array([hm.overlap_stereo(r[0], r[1], r[2], r[3], float(ins["cfg"][5])) for r in ins["table"]], np.float64)
    assert bits(got) == bits(ref["out"]), np.flatnonzero(got.view(np.int64) != ref["out"].view(np.int64))[:5]
    ins, ref = S.load_fixture("filter")
    got = np.array([hm.filter_disparity(r[0], r[2], r[4], r[6], float(ins["cfg"][7])) for r in ins["table"]], np.float64)
    assert bits(got) == bits(ref["out"]), np.flatnonzero((got.view(np.int64) != ref["out"].view(np.int64)).any(1))[:5]


# ------------------------------------------------------------------------------------------------------- the descriptor matchers
@pytest.mark.parametrize("name", NNR + MATCH)
def test_descriptor_matchers_equal_the_reference(po, name):
    ins, ref = S.load_fixture(name)
    d1, d2 = S.descriptor_inputs(name)
    nnr = float(ins["params"][0])
    if name.startswith("nnr_"):
        results = (("restatement", hm.match_nnr(d1, d2, nnr)), ("oracle", po.match_nnr(d1, d2, nnr)))
    else:
        lr = bool(ins["params"][1])
        results = (("restatement", hm.match_lines(d1, d2, nnr, lr)), ("oracle", po.match_lines(d1, d2, nnr, lr)))
    for who, (n, m) in results:
        assert n == int(ref["ret"][0]) and m.dtype == np.int32 and bits(m) == bits(ref["m12"]), (name, who)
    # the two nearest train rows behind an accepted match (the stand-in's knnMatch breaks equal distances to the lower train row)
    idx, _ = hm.knn2(d1, d2)
    oidx, _ = po.knn2(d1, d2)
    ok = ref["m12"] >= 0
    assert np.array_equal(idx, oidx) and np.array_equal(idx[ok, 0], ref["m12"][ok])


@pytest.mark.parametrize("name", DIST)
def test_descriptor_distance_equals_the_reference(po, name):
    ins, ref = S.load_fixture(name)
    assert bits(hm.hamming(ins["a"], ins["b"])) == bits(ref["out"]) == bits(po.descriptor_distance(ins["a"], ins["b"]))


def test_stereo_from_rgbd_equals_the_reference(po):
    ins, ref = S.load_fixture("rgbd")
    kp = np.zeros(len(ins["kp"]), hm.KEYPOINT_DT)
    kp["x"], kp["y"] = ins["kp"][:, 0], ins["kp"][:, 1]
    ur, dp = po.stereo_from_depth(kp, ins["depth_image"], float(ins["rig"][1]))
    assert bits(ur) == bits(ref["uright"]) and bits(dp) == bits(ref["depth"])
    assert (ref["depth"] > 0).sum() > 30 and (ref["depth"] < 0).sum() > 20


# --------------------------------------------------------------------------------------------------------------------- mutants
POINT_SWITCHES = ["band_end_exclusive", "vl_rounded", "endu_gt", "orb_le", "median_low", "cut_le", "ur_bounds_exclusive",
                  "octave_gate_narrow", "maxd_inclusive", "hamming_to_vdistidx"]
LINE_SWITCHES = ["nan_dir_rejected", "col_equal_kept", "ratio_float", "epr_from_old_spr", "length_eln_sln"]
TABLE_SWITCHES = ["length_eln_sln", "overlap_zero_horizontal"]
UNREJECTABLE = ["ul_minus_001_float", "sort_ties_insertion", "nan_minmax"]          # (the module docstring says why)


def _mut(rule):
    return replace(hm.REF, **{rule: "fmin" if rule == "nan_minmax" else True})


def test_every_switch_is_held_to_the_rule():
    assert sorted(set(POINT_SWITCHES + LINE_SWITCHES + TABLE_SWITCHES + UNREJECTABLE)) == sorted(f.name for f in fields(hm.Rules))


@pytest.mark.parametrize("rule", POINT_SWITCHES)
def test_a_mutated_point_rule_differs_from_a_reference_fixture(po, rule):
    small_first = sorted((n for n in POINTS if "pair" not in n and "same" not in n and "pipeline" not in n), key=lambda n: len(S.load_fixture(n)[0]["kpL"]))
    for name in small_first + [n for n in POINTS if n not in small_first]:
        c, ref = case(po, name)
        ur, dp = hm.run_points(c, _mut(rule))[:2]
        if bits(ur) != bits(ref["uright"]) or bits(dp) != bits(ref["depth"]):
            print(rule, "rejected by", name)
            return
    pytest.fail("no reference fixture tells the mutant %s from the reference's rule" % rule)


@pytest.mark.parametrize("rule", LINE_SWITCHES)
def test_a_mutated_line_rule_differs_from_a_reference_fixture(po, rule):
    for name in LINES:
        c, ref = case(po, name)
        disp, le, _, _ = hm.stereo_lines(c["cfg"], c["klL"], c["ldL"], c["klR"], c["ldR"], c["W"], c["H"], _mut(rule))
        if bits(disp) != bits(ref["disp"]) or bits(le) != bits(ref["le"]):       # what the device record carries
            print(rule, "rejected by", name)
            return
    pytest.fail("no reference fixture tells the mutant %s from the reference's rule" % rule)


@pytest.mark.parametrize("rule", TABLE_SWITCHES)
def test_a_mutated_overlap_rule_differs_from_the_reference_table(rule):
    ins, ref = S.load_fixture("overlap")
    got = np.array([hm.overlap_stereo(r[0], r[1], r[2], r[3], float(ins["cfg"][5]), _mut(rule)) for r in ins["table"]], np.float64)
    assert bits(got) != bits(ref["out"]), "the overlap fixture cannot tell the mutant %s from the reference's rule" % rule


@pytest.mark.parametrize("rule", UNREJECTABLE)
def test_a_switch_no_table_can_reject_changes_nothing(po, rule):
    for name in POINTS:
        c, ref = case(po, name)
        ur, dp = hm.run_points(c, _mut(rule))[:2]
        assert bits(ur) == bits(ref["uright"]) and bits(dp) == bits(ref["depth"]), (rule, name)
    for name in LINES:
        c, ref = case(po, name)
        disp, le, m12, _ = hm.stereo_lines(c["cfg"], c["klL"], c["ldL"], c["klR"], c["ldR"], c["W"], c["H"], _mut(rule))
        assert bits(disp) == bits(ref["disp"]) and bits(le) == bits(ref["le"]) and bits(m12) == bits(ref["m12"]), (rule, name)
    ins, ref = S.load_fixture("overlap")
    assert np.isnan(ins["table"]).any(1).sum() >= 3
    got = np.array([hm.overlap_stereo(r[0], r[1], r[2], r[3], float(ins["cfg"][5]), _mut(rule)) for r in ins["table"]], np.float64)
    assert bits(got) == bits(ref["out"])
    ins, ref = S.load_fixture("filter")
    assert np.isnan(ins["table"]).any(1).sum() >= 10
    got = np.array([hm.filter_disparity(r[0], r[2], r[4], r[6], float(ins["cfg"][7]), _mut(rule)) for r in ins["table"]], np.float64)
    assert bits(got) == bits(ref["out"])


# ------------------------------------------------------------------------------------------------------------------------ area
@pytest.mark.parametrize("name", AREA)
def test_features_in_area_equal_the_restatements(name):
    """Frame::AssignFeaturesToGrid / PosInGrid / GetFeaturesInArea of the reference against helpers_matchers._cells / _area, the Python
    statement the matcher pins rest on: every list, order included, one camera and two."""
    ins, ref = S.load_fixture(name)
    lists = S.area_restated(ins)
    start, idx = ref["start"], ref["idx"]
    assert len(start) == len(lists) + 1 and start[-1] == len(idx)
    nonempty = 0
    for i, want in enumerate(lists):
        got = idx[start[i]:start[i + 1]]
        assert np.array_equal(got, want), (name, i, ins["q"][i], got[:8], want[:8])
        nonempty += len(got) > 1
    assert nonempty > 60
    if int(ins["nleft"][0]) != -1:
        assert (ins["q"][:, 5] != 0).sum() > 40 and (ins["q"][:, 5] == 0).sum() > 40


def _match_program_has_area():
    import helpers_match_ref as HMR
    if not os.path.exists(HMR.REF_EXE):
        return False
    import subprocess
    r = subprocess.run([HMR.REF_EXE, "--functions"], capture_output=True, text=True, timeout=60)
    return r.returncode == 0 and "area" in r.stdout.split()


@pytest.mark.skipif(not _match_program_has_area(), reason="oracle/_ref/pli_ref_match with `area` is built only where the reference tree exists")
@pytest.mark.parametrize("name", AREA)
def test_features_in_area_equal_the_stand_in_of_the_matcher_pin(name):
    """The C++ restatement the matcher pins were recorded over (match_shim: ShimTable::AssignFeaturesToGrid[TwoCameras] and area(),
    through pli_ref_match's own `area`) returns what the reference's Frame.cc returned, list by list, order included."""
    import helpers_match_ref as HMR
    ins, ref = S.load_fixture(name)
    got = HMR.run_reference(dict(fn=np.frombuffer(b"area", np.uint8), **{k: ins[k] for k in ("kp", "nleft", "bounds", "q")}))
    assert got["start"].tobytes() == ref["start"].tobytes() and got["idx"].tobytes() == ref["idx"].tobytes(), name


# ----------------------------------------------------------------------------------- what was removed for the reference, and coverage
def test_dropped_rows_carry_exactly_the_undefined_labels(po):
    """Rebuilds the cases as they were before anything was removed: the rows missing from a fixture are exactly the rows whose label
    is one the reference has no defined behaviour for; a missing case is one whose vDistIdx is empty."""
    man = S.manifest()
    originals = {"points_" + c["name"]: c for c in S.point_cases(po) + [S.pipeline_case(po)]}
    assert set(POINTS) | set(man["dropped_cases"]) == set(originals) and not set(POINTS) & set(man["dropped_cases"])
    for name, why in man["dropped_cases"].items():
        assert why == S.UNDEFINED_FRAME_TAG and S.UNDEFINED_FRAME_TAG in hm.run_points(_without_undefined_rows(originals[name]))[5]
    ndrop = 0
    for name in POINTS:
        o = originals[name]
        ins = S.load_fixture(name)[0]
        assert S.right_band_outside(o).tolist() == ins["dropped_right"].tolist() == []
        ex = hm.run_points(o)[4]
        undefined = [i for i, e in enumerate(ex) if e[0] in S.UNDEFINED_POINT_EXITS]
        assert undefined == ins["dropped_left"].tolist(), name
        assert man["dropped_left_rows"].get(name, {}) == {str(i): ex[i][0] for i in undefined}
        keep = np.setdiff1d(np.arange(len(o["kpL"])), undefined)
        assert bits(o["kpL"][keep]) == bits(ins["kpL"]) and bits(o["descL"][keep]) == bits(ins["descL"])
        assert bits(o["kpR"]) == bits(ins["kpR"]) and bits(o["descR"]) == bits(ins["descR"])
        r = hm.run_points(case(po, name)[0])
        assert not [e for e in r[4] if e[0] in S.UNDEFINED_POINT_EXITS] and S.UNDEFINED_FRAME_TAG not in r[5], name
        ndrop += len(undefined)
    assert ndrop >= 20
    for name in NNR + MATCH:                      # matches_[idx][1] exists: two train rows, both ways for match
        d1, d2 = S.descriptor_inputs(name)
        assert len(d2) >= 2 and (name.startswith("nnr_") or len(d1) >= 2), name


def _without_undefined_rows(c):
    ex = hm.run_points(c)[4]
    keep = [i for i, e in enumerate(ex) if e[0] not in S.UNDEFINED_POINT_EXITS]
    return dict(c, kpL=c["kpL"][keep], descL=c["descL"][keep])


def test_coverage_of_the_reference_cases(po):
    cov = S.coverage(po)
    print(json.dumps(cov, indent=1, sort_keys=True))
    S.check_coverage(cov)
    assert cov == S.manifest()["coverage"]


# ------------------------------------------------------------------------------------------------------------------------ live
LIVE = set(S.FUNCTIONS) <= set(S.reference_functions())


@pytest.mark.skipif(not LIVE, reason="oracle/_ref/pli_ref_stereo is built only where the reference tree exists (or lists fewer functions)")
def test_live_reference_equals_every_fixture(po):
    """Rebuilds every case, reruns it through the program and compares inputs and results with the committed files byte for byte."""
    fixtures, man = S.build_all(po)
    assert sorted(fixtures) == NAMES
    for k in ("dropped_cases", "dropped_left_rows", "dropped_right_rows"):
        assert man[k] == S.manifest()[k]
    assert S.generate(po, write=False) == []
