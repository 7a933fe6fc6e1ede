"""The stereo matchers and the descriptor matchers against tests/helpers_matchers.py, a restatement written from the
reference's text in a different shape than oracle/match_oracle.hpp (CPU only; the GPU side is test_independent_matchers_gpu.py).

Every comparison is equality: every quantity is an integer or an IEEE float expression with a fixed order.  No case and no
query is left out.  Coverage is asserted with the labels the restatement returns.

Struck from the lists of exits (helpers_matchers.POINT_LABELS_UNREACHABLE / LINE_LABELS_UNREACHABLE), with the reason:
  * deltaR = NaN / +-inf, |deltaR| > 1 and deltaR == +-1.  The sliding window keeps the FIRST strict minimum of the eleven SADs
    and leaves when it sits at an end.  So at an interior best, dist1 > dist2 (else dist1 would have been kept) and
    dist3 >= dist2.  SADs are integers below 2^16, exact in float, so with a = dist1 - dist2 >= 1 and b = dist3 - dist2 >= 0
    the denominator 2 (a + b) is positive and deltaR = (a - b) / (2 (a + b)) lies in [-0.5, 0.5].  `deltaR < -1 || deltaR > 1`
    is dead code on any table, and so is the difference between rejecting a NaN early or late: that mutation is not run.
    What can be reached is deltaR == +-0.5 (one neighbour equal to the best), which is in the list instead.
  * `uL - 0.01` in float instead of double: the same float for every uL >= 4.5, which the left window requires; see
    test_ul_minus_001_in_float_or_in_double_is_the_same_float.  That mutation is not run either.
  * "right line horizontal" as a rejection of its own: sp_r(1) and ep_r(1) are overwritten with the left line's rows before
    `abs(sp_r(1) - ep_r(1)) > lineHorizTh` is read, so that test repeats the left line's.  The division by zero itself is
    reached (label right_horizontal_division_by_zero) and shown not to reach any output, under std::min and under fmin.
"""
from dataclasses import replace

import numpy as np
import pytest

import helpers_matchers as hm
from pli_slam_amd import synth

W, H = 752, 480


@pytest.fixture(scope="session")
def po():
    from oracle import pyoracle
    pyoracle.lib()
    return pyoracle


def ocfg(po, W, H, **over):
    return po.default_config(W, H, **over)


def corpus(po):
    return hm.stereo_corpus(po)


run_points = hm.run_points


def oracle_points(po, c):
    return po.stereo_points_tables(c["cfg"], c["kpL"], c["descL"], c["kpR"], c["descR"], c["pyr"][0], c["pyr"][1])


def points_equal(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a[:4], b[:4]))


def lines_equal(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a[:3], b[:3]))


def test_restatement_equals_oracle_stereo_points(po):
    n = 0
    for c in corpus(po):
        if c["pyr"] is None:
            continue
        got, want = run_points(c), oracle_points(po, c)
        for name, g, w in zip(("uright", "depth", "best_idx", "sad"), got, want):
            bad = np.flatnonzero(g.view(np.int32) != w.view(np.int32))
            assert bad.size == 0, "%s: %s differs at left keypoints %s (exits %s)" % (c["name"], name, bad[:5], [got[4][i] for i in bad[:5]])
        n += len(c["kpL"])
    assert n > 4000


def test_oracle_table_entry_equals_its_frame_path(po):
    """stereo_points_tables on the pipeline's own tables == Frame.stereo_points()."""
    L, R = synth.make_stereo_pair(0, W, H)
    cfg = ocfg(po, W, H)
    fr = po.Frame(cfg)
    t = {}
    for eye, img, k in ((0, L, "L"), (1, R, "R")):
        _, t["kp" + k], t["desc" + k] = fr.orb_extract(eye, img)
    pyr = [[fr.pyramid(e, l) for l in range(8)] for e in (0, 1)]
    a = fr.stereo_points()
    b = po.stereo_points_tables(cfg, t["kpL"], t["descL"], t["kpR"], t["descR"], pyr[0], pyr[1])
    assert points_equal(a, b) and (a[0] >= 0).sum() > 300


def test_oracle_table_entry_refuses_rows_outside_the_image(po):
    c = [c for c in corpus(po) if c["name"] == "const_curves"][0]
    for field, val in (("y", -1.0), ("y", float(H)), ("y", np.nan), ("octave", 8), ("octave", -1)):
        kp = c["kpL"].copy(); kp[field][0] = val
        with pytest.raises(ValueError):
            po.stereo_points_tables(c["cfg"], kp, c["descL"], c["kpR"], c["descR"], c["pyr"][0], c["pyr"][1])


def test_restatement_equals_oracle_stereo_lines(po):
    n = 0
    for c in corpus(po):
        got = hm.stereo_lines(c["cfg"], c["klL"], c["ldL"], c["klR"], c["ldR"], c["W"], c["H"])
        want = po.stereo_lines_tables(c["cfg"], c["klL"], c["ldL"], c["klR"], c["ldR"], c["W"], c["H"])
        for name, g, w in zip(("disp", "le", "m12"), got, want):
            assert g.tobytes() == w.tobytes(), "%s: %s differs at left lines %s" % (
                c["name"], name, np.flatnonzero((g.reshape(len(g), -1) != w.reshape(len(w), -1)).any(1))[:5])
        # std::min / std::max against fmin / fmax: they treat NaN differently; no output depends on it
        alt = hm.stereo_lines(c["cfg"], c["klL"], c["ldL"], c["klR"], c["ldR"], c["W"], c["H"], replace(hm.REF, nan_minmax="fmin"))
        assert lines_equal(got, alt), c["name"]
        n += len(c["klL"])
    assert n > 500


def labels(po):
    pts, lns = {}, {}
    for c in corpus(po):
        if c["pyr"] is not None:
            r = run_points(c)
            for e in r[4]:
                for t in e:
                    pts[t] = pts.get(t, 0) + 1
            if len(c["kpL"]):
                for t in r[5]:
                    pts[t] = pts.get(t, 0) + 1
        for e in hm.stereo_lines(c["cfg"], c["klL"], c["ldL"], c["klR"], c["ldR"], c["W"], c["H"])[3]:
            for t in e:
                lns[t] = lns.get(t, 0) + 1
    return pts, lns


def test_every_exit_is_reached(po):
    pts, lns = labels(po)
    print("stereo points:", sorted(pts.items()))
    print("stereo lines:", sorted(lns.items()))
    missing = [l for l in hm.POINT_LABELS if not pts.get(l)] + [l for l in hm.LINE_LABELS if not lns.get(l)]
    assert not missing, "exits the corpus does not reach: %s" % missing
    # what was struck really does not occur
    assert not [l for l in hm.POINT_LABELS_UNREACHABLE if pts.get(l)] and not [l for l in hm.LINE_LABELS_UNREACHABLE if lns.get(l)]


POINT_MUTANTS = ["band_end_exclusive", "vl_rounded", "endu_gt", "orb_le", "median_low", "cut_le", "ur_bounds_exclusive",
                 "octave_gate_narrow", "maxd_inclusive"]
LINE_MUTANTS = ["nan_dir_rejected", "col_equal_kept", "ratio_float"]


@pytest.mark.parametrize("rule", POINT_MUTANTS)
def test_a_mutated_point_rule_disagrees_with_the_oracle(po, rule):
    """(NaN deltaR rejected early or late is not among them: NaN cannot occur, see the module docstring.)"""
    bad = [c["name"] for c in corpus(po) if c["pyr"] is not None and c["name"].split("_")[0] != "pipeline"
           and not points_equal(run_points(c, replace(hm.REF, **{rule: True})), oracle_points(po, c))]
    print(rule, "caught by", bad)
    assert bad, "the corpus cannot tell the mutant %s from the reference's rule" % rule


@pytest.mark.parametrize("rule", LINE_MUTANTS)
def test_a_mutated_line_rule_disagrees_with_the_oracle(po, rule):
    bad = []
    for c in corpus(po):
        if c["name"].startswith("pipeline"):
            continue
        got = hm.stereo_lines(c["cfg"], c["klL"], c["ldL"], c["klR"], c["ldR"], c["W"], c["H"], replace(hm.REF, **{rule: True}))
        want = po.stereo_lines_tables(c["cfg"], c["klL"], c["ldL"], c["klR"], c["ldR"], c["W"], c["H"])
        if not lines_equal(got[:2], want[:2]):          # disp and le: what the device record carries (m12 alone does not count)
            bad.append(c["name"])
    print(rule, "caught by", bad)
    assert bad, "the corpus cannot tell the mutant %s from the reference's rule" % rule


def test_ul_minus_001_in_float_or_in_double_is_the_same_float():
    """`bestuR = uL - 0.01` is evaluated in double.  A float evaluation (uL - 0.01f) rounds to the same float for every uL that
    can get there: the left window needs round(uL / scale) >= 5, so uL >= 4.5.  0.01f is 2.2e-10 below 0.01; inside one binade
    uL - 0.01 sits at a fixed offset from the rounding boundaries (uL is a multiple of the ulp), at least 9e-9 from them for
    results in [4, 2048), so 2.2e-10 never crosses one.  Checked here on every float of [2^k, 2^k + 0.02) (results that fall
    into the finer binade below) and on a stride through the rest.  Hence no table can tell this mutant apart, the mutation
    test is not run, and the kernel's double subtraction is pinned by the reference's text alone."""
    f = np.float32
    for k in range(2, 11):
        lo = np.array(2.0 ** k, f).view(np.uint32)
        n = int(np.array(2.0 ** k + 0.02, f).view(np.uint32) - lo) + 1
        dense = (lo + np.arange(n, dtype=np.uint32)).view(f)
        stride = (lo + np.arange(0, 1 << 23, 97, dtype=np.uint32)).view(f)
        for u in (dense, stride):
            u = u[u >= 4.5]
            assert np.array_equal((u - f(0.01)).astype(f), (u.astype(np.float64) - 0.01).astype(f))


def test_validator_refuses_what_the_kernels_may_not_be_given(po):
    c = [c for c in corpus(po) if c["name"] == "const_curves"][0]
    base = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    assert hm.validate_tables(base, kp_cap=2000, kl_cap=200) is base
    def broken(key, field, val):
        d = dict(base); d[key] = base[key].copy(); d[key][field][0] = val
        return d
    for d in (broken("kpL", "octave", 8), broken("kpR", "octave", -1), broken("kpL", "x", np.inf), broken("kpR", "y", np.nan),
              broken("kpL", "y", -0.5 - 1), broken("kpR", "y", float(H)), broken("kpL", "x", 3.0e9)):
        with pytest.raises(ValueError):
            hm.validate_tables(d)
    with pytest.raises(ValueError):
        hm.validate_tables(base, kp_cap=len(base["kpL"]) - 1)
    lc = [c for c in corpus(po) if c["name"] == "lines_geometry"][0]
    with pytest.raises(ValueError):
        hm.validate_tables(lc, kl_cap=3)
    d = dict(lc); d["klR"] = lc["klR"].copy(); d["klR"]["endPointX"][0] = np.nan
    with pytest.raises(ValueError):
        hm.validate_tables(d)
    d = dict(lc); d["klL"] = lc["klL"].copy(); d["klL"]["startPointY"][0] = 1.0e7
    with pytest.raises(ValueError):
        hm.validate_tables(d)


def test_descriptor_matchers_equal_the_oracle(po):
    a, b, c, d = hm.descriptor_tables_random_and_ties()
    idx, dist = hm.knn2(a, b)
    oidx, odist = po.knn2(a, b)
    assert np.array_equal(idx, oidx) and np.array_equal(dist, odist)
    for q, t in ((a, b), (c, d), (a[:3], b[:1]), (a[:5], b[:2]), (a[:0], b)):
        for nnr in (0.9, 0.75, 1.0):
            n, m = hm.match_nnr(q, t, nnr)
            on, om = po.match_nnr(q, t, nnr)
            assert n == on and np.array_equal(m, om)
            for lr in (True, False):
                n, m = hm.match_lines(q, t, nnr, lr)
                on, om = po.match_lines(q, t, nnr, lr)
                assert n == on and np.array_equal(m, om)
    # nnratio products at the float boundary
    seen = set()
    for q, t, d0, d1 in hm.nnr_float_boundary_tables():
        for nnr in (0.9, 0.6):
            n, m = hm.match_nnr(q, t, nnr)
            on, om = po.match_nnr(q, t, nnr)
            assert n == on and np.array_equal(m, om), (d0, d1, nnr)
            assert (n == 1) == bool(np.float32(d0) < np.float32(np.float32(d1) * np.float32(nnr)))
            if float(d0) == float(np.float32(np.float32(d1) * np.float32(nnr))):
                seen.add("equal")
            if (d0 < d1 * float(nnr)) != (n == 1):
                seen.add("float_differs_from_double")
    assert seen == {"equal", "float_differs_from_double"}


# ---- the projection searches ---------------------------------------------------------------------------------------------------
def proj_runs(c):
    for occ in (None, c["occ"]):
        for ori in (True, False):
            yield occ, ori


def test_projection_searches_equal_the_oracle_on_constructed_cases(po):
    """Distance exactly at TH_HIGH; level gates at both ends; the uright gate present / absent / at |error| == radius; occupied
    keypoints; map points without observations; the three ComputeThreeMaxima outcomes; rot at multiples of 12 degrees, at 360 and
    at the real bin boundaries 15 + 30 k (factor = 1 / HISTO_LENGTH makes the bins 30 degrees wide); windows with exactly PROJ_K
    and PROJ_K + 1 candidates; nnratio products at the float boundary.  Coverage asserted with the restatement's labels."""
    seen_p, seen_l = set(), set()
    for c in hm.build_projection_cases():
        for occ, ori in proj_runs(c):
            n, best, raw, ex, ct = hm.search_by_projection(c["q"], c["qd"], c["kp"], c["desc"], c["ur"], c["bounds"], ori, occ)
            on, obest, oraw = po.search_by_projection(c["q"], c["qd"], c["kp"], c["desc"], c["ur"], c["bounds"], ori, occupied=occ, with_raw=True)
            assert n == on and np.array_equal(best, obest) and np.array_equal(raw, oraw), (c["name"], occ is not None, ori)
            seen_p |= ct | {t for e in ex for t in e}
        for occ in (None, c["occ"]):
            for nnratio in (0.8, 0.5, 1.0):
                n, best, ex = hm.search_local_map(c["q"], c["qd"], c["kp"], c["desc"], c["ur"], occ, c["bounds"], nnratio)
                on, obest = po.search_local_map(c["q"], c["qd"], c["kp"], c["desc"], c["ur"], occ, c["bounds"], nnratio)
                assert n == on and np.array_equal(best, obest), (c["name"], occ is not None, nnratio)
                seen_l |= {t for e in ex for t in e}
    missing = [l for l in hm.PROJ_LABELS if l not in seen_p] + ["local map: " + l for l in hm.LOCAL_MAP_LABELS if l not in seen_l]
    assert not missing, "exits the projection cases do not reach: %s" % missing


def test_projection_searches_equal_the_oracle_on_the_random_generators(po):
    q, qd, kp, desc, ur, bounds = hm.local_map_ties_tables()
    for nnratio in (0.8, 0.5, 1.0):
        n, best, _ = hm.search_local_map(q, qd, kp, desc, ur, None, bounds, nnratio)
        on, obest = po.search_local_map(q, qd, kp, desc, ur, None, bounds, nnratio)
        assert n == on and np.array_equal(best, obest)
    q, qd, kp, desc, ur, occ, bounds, rng = hm.dense_window_tables(3000, 1500)
    for nnratio in (0.8, 0.3):
        n, best, _ = hm.search_local_map(q, qd, kp, desc, ur, occ, bounds, nnratio)
        on, obest = po.search_local_map(q, qd, kp, desc, ur, occ, bounds, nnratio)
        assert n == on and np.array_equal(best, obest)
    qn = q.copy()
    qn["valid"] = np.where((qn["valid"] != 0) & (rng.random(len(q)) < 0.4), 3, qn["valid"])
    for qq, oc in ((q, None), (qn, occ)):
        for ori in (True, False):
            n, best, raw, _, _ = hm.search_by_projection(qq, qd, kp, desc, ur, bounds, ori, oc)
            on, obest, oraw = po.search_by_projection(qq, qd, kp, desc, ur, bounds, ori, occupied=oc, with_raw=True)
            assert n == on and np.array_equal(best, obest) and np.array_equal(raw, oraw) and on > 75


def test_three_maxima_against_the_sequential_definition():
    """ComputeThreeMaxima as the reference writes it (one pass, three running maxima) against the sort used by the restatement."""
    rng = np.random.default_rng(3)
    for _ in range(2000):
        sizes = rng.integers(0, rng.integers(1, 40), 30).tolist()
        m1 = m2 = m3 = 0; i1 = i2 = i3 = -1
        for i, s in enumerate(sizes):
            if s > m1:
                m3, m2, m1, i3, i2, i1 = m2, m1, s, i2, i1, i
            elif s > m2:
                m3, m2, i3, i2 = m2, s, i2, i
            elif s > m3:
                m3, i3 = s, i
        if m2 < np.float32(0.1) * np.float32(m1):
            i2 = i3 = -1
        elif m3 < np.float32(0.1) * np.float32(m1):
            i3 = -1
        assert hm.three_maxima(sizes)[0] == [i1, i2, i3], sizes
