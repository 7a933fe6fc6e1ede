"""Pins the oracle's ORB extractor to the reference's own src/ORBextractor.cc.

tests/golden/orb_ref/*.npz hold what ORB_SLAM3::ORBextractor::operator() itself returned for every case of
tests/helpers_orb_ref.py: the reference's translation unit compiled where it lies against oracle/ref_recipe/cv_shim/, with the
four OpenCV primitives it calls (FAST, GaussianBlur, resize, copyMakeBorder) backed by oracle/ocv_prims.hpp, run by
oracle/_ref/pli_ref_orb under a monotone heap (tools/gen_orb_ref.py).  What is pinned is the reference's control flow, geometry
and arithmetic: cell geometry, the two-threshold fallback, the per-level quotas, DistributeOctTree with its list order and its
sort, the rescale to level 0, IC_Angle, the steered BRIEF and the lapping order.  OpenCV's own bit conventions are not (those
stay with tools/pin/run_pin.sh).  Every comparison is byte equality over every row of every case.
"""
import os

import numpy as np
import pytest

import helpers_orb_ref as H

REF_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref")
REF_EXE = os.path.join(REF_DIR, "pli_ref_orb")
REF_EXE_SYSHEAP = os.path.join(REF_DIR, "pli_ref_orb_sysheap")

# the labels each constructed case was built to reach (OrbCoverage in oracle/orb_oracle.hpp), beside the corpus-wide check
BUILT_FOR = {
    "dots_split_lines_240": ["keys_on_split_line", "stop_all_single"],
    "dots_thresholds_seams_240": ["fallback_cells", "mixed_cells", "seam_pairs", "stop_all_single"],
    "dots_equal_maxima_240": ["equal_maxima", "stop_quota_expand"],
    "noise_budget12_240": ["stop_quota_expand"],
    "dots_tie_groups_376x240": ["sort_ties", "tie_split_at_break", "stop_quota_break"],
    "dots_ini_boundary_640x240": ["keys_on_ini_boundary"],
    "dots_low_thresholds_240": ["fallback_cells", "mixed_cells"],
    "noise_high_thresholds_240": ["fallback_cells", "mixed_cells"],
    "noise_skip_column_813x240_l2": ["skipped_cells", "clipped_cells"],
    "dots_narrow_row_440x813_l2": ["narrow_cells"],
    "dots_7px_column_814x240_l2": ["seven_px_cells"],
    "dots_7px_row_440x814_l2": ["seven_px_cells"],
    "dots_skip_row_470x903_l2": ["skipped_cells"],
}


def _frame(oracle, p):
    cfg = oracle.default_config(p.W, p.H, orb_nfeatures=p.nfeatures, orb_scale_factor=p.scale_factor, orb_nlevels=p.nlevels,
                                orb_ini_th_fast=p.ini_th, orb_min_th_fast=p.min_th)
    return oracle.Frame(cfg)


def _assert_rows_equal(kp, desc, fix, what):
    assert len(kp) == len(fix["kp"]), (what, "keypoint count", len(kp), len(fix["kp"]))
    assert kp.tobytes() == fix["kp"].tobytes(), (what, "keypoints differ from the reference's")
    assert np.array_equal(desc, fix["desc"]), (what, "descriptors differ from the reference's")


@pytest.fixture(scope="module")
def oracle_runs(oracle):
    """One oracle run per case, shared: {name: (n, mono, kp, desc, per-level coverage, pyramid levels or None)}."""
    out = {}
    for p, cases in H.groups():
        fr = _frame(oracle, p)
        for c in cases:
            img = c.image()
            n, mono, kp, desc = fr.orb_extract_lapping(0, img, c.lapping)
            cov = [fr.level_coverage(0, l) for l in range(p.nlevels)]
            levels = [fr.pyramid(0, l) for l in range(p.nlevels)] if c.pyramid else None
            plain = fr.orb_extract(0, img) if c.lapping == (0, 0) else None
            out[c.name] = (n, mono, kp, desc, cov, levels, plain)
    return out


def test_corpus_has_the_required_cases():
    names = [c.name for c in H.CASES]
    assert sorted(os.listdir(H.GOLD_DIR)) == sorted(n + ".npz" for n in names)
    assert sum(c.pyramid for c in H.CASES) == 3
    assert {c.params.nfeatures for c in H.CASES} >= {12, 300, 1200}
    assert {(c.params.nlevels, c.params.scale_factor) for c in H.CASES} >= {(4, 2.0), (12, 1.1), (8, 1.2)}
    assert {(c.params.ini_th, c.params.min_th) for c in H.CASES} >= {(5, 2), (80, 40), (20, 7)}
    assert all(c.params.W * c.params.H < 752 * 480 or c.params.nlevels == 2 for c in H.CASES)
    # lapping intervals that send none, some and all keypoints to the tail
    share = [(H.load_fixture(c.name)["mono"], len(H.load_fixture(c.name)["kp"])) for c in H.CASES]
    assert all(n > 0 for _, n in share)
    assert any(m == n for m, n in share) and any(0 < m < n for m, n in share) and any(m == 0 for m, n in share)


@pytest.mark.parametrize("case", H.CASES, ids=lambda c: c.name)
def test_oracle_equals_reference_fixture(oracle_runs, case):
    fix = H.load_fixture(case.name)
    n, mono, kp, desc, _, levels, plain = oracle_runs[case.name]
    assert n == len(fix["kp"]) and mono == fix["mono"], (n, mono, fix["mono"])
    _assert_rows_equal(kp, desc, fix, "orb_extract_lapping")
    if plain is not None:                                    # vLappingArea = {0, 0}: the table orb_extract itself returns
        assert plain[0] == fix["mono"]
        _assert_rows_equal(plain[1], plain[2], fix, "orb_extract")
    assert (levels is not None) == (fix["levels"] is not None) == case.pyramid
    if case.pyramid:
        assert len(levels) == len(fix["levels"]) == case.params.nlevels
        for l, (a, b) in enumerate(zip(levels, fix["levels"])):
            assert a.shape == b.shape and np.array_equal(a, b), ("pyramid level", l)


@pytest.mark.skipif(not os.path.exists(REF_EXE), reason="oracle/_ref/pli_ref_orb is built only where the reference tree exists")
@pytest.mark.parametrize("case", H.CASES, ids=lambda c: c.name)
def test_live_reference_equals_fixture(case):
    fix = H.load_fixture(case.name)
    res = H.run_reference(REF_EXE, case)
    assert res["mono"] == fix["mono"]
    _assert_rows_equal(res["kp"], res["desc"], fix, "live reference run")
    assert len(res["levels"]) == case.params.nlevels
    if case.pyramid:
        for l, (a, b) in enumerate(zip(res["levels"], fix["levels"])):
            assert a.shape == b.shape and np.array_equal(a, b), ("pyramid level", l)


def test_corpus_reaches_every_branch(oracle, oracle_runs):
    """Coverage is asserted, not assumed: every counter of OrbCoverage is reached somewhere in the corpus, nIni takes 1, 2 and 3,
    every level of every case is inside the contract, and each constructed case reaches what it was constructed for."""
    total, ninis = {}, set()
    for c in H.CASES:
        per_case = {}
        for cov in oracle_runs[c.name][4]:
            assert cov["nIni"] >= 1, (c.name, "a level outside the contract")
            ninis.add(cov["nIni"])
            for k, v in cov.items():
                if k != "nIni":
                    per_case[k] = per_case.get(k, 0) + v
                    total[k] = total.get(k, 0) + v
        for k in BUILT_FOR.get(c.name, []):
            assert per_case[k] > 0, (c.name, k, per_case)
    assert len(total) == 15 and all(v > 0 for v in total.values()), total
    assert ninis >= {1, 2, 3}, ninis
    assert set(BUILT_FOR) <= set(H.CASE_BY_NAME)


@pytest.mark.skipif(not os.path.exists(REF_EXE_SYSHEAP), reason="oracle/_ref/pli_ref_orb_sysheap is built only where the reference tree exists")
def test_sysheap_report():
    """The reference under the C library's heap: DistributeOctTree orders equal node sizes by heap address (ORBextractor.cc:682),
    so this binary need not reproduce the fixtures, or itself on another C library.  Nothing about equality is asserted: the
    share of differing rows per case is reported (pytest -s) and DESIGN.md §2 holds the measured table."""
    print()
    for c in H.CASES:
        res = H.run_reference(REF_EXE_SYSHEAP, c)
        bad, total = H.differing_rows(res, H.load_fixture(c.name))
        print("sysheap %-36s %5d / %5d rows differ (%5.1f %%), %5d keypoints, the fixture %5d" % (
            c.name, bad, total, 100.0 * bad / max(total, 1), len(res["kp"]), len(H.load_fixture(c.name)["kp"])))
        assert len(res["levels"]) == c.params.nlevels           # the run completed and answered in the expected form
