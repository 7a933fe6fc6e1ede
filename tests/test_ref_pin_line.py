"""The line path pinned to the reference's own compiled code: LSDDetectorC::detectImpl(..., LSDOptions, ...) (clamps, float/double
length, the min_length gate, every KeyLine field), Lineextractor::operator() (std::sort by response, the cut, the re-numbering),
BinaryDescriptor::compute / computeImpl / computeSobel / computeLBD / binaryConversion and the weight tables.

tests/golden/line_ref holds what oracle/_ref/pli_ref_line and pli_ref_line_mathh returned (the reference's four translation units
compiled where they lie; see oracle/Makefile and tests/helpers_line_ref.py).  Here the oracle's restatement must equal those recorded
bytes in every key-line field, both descriptor forms and the gradient planes; where the reference tree is present the two programs
are run again and must reproduce the fixtures; a Python restatement with one deliberate misreading at a time must be rejected; and
the branches the corpus was built for are counted from the fixtures.

What the pin covers: control flow and arithmetic BETWEEN four primitives (LineSegmentDetector::detect, LineIterator, GaussianBlur,
Sobel), which the driver defines over the oracle's own restatements.  The detector itself and OpenCV's bit conventions stay with
tools/pin/run_pin.sh.

Overloads (measured here, recorded in DESIGN.md "Oracle"): the two programs agree on every case, and both select the FLOAT overloads of
the unqualified cos / sin (binary_descriptor_custom.cpp:1130-1131) and atan2 (LSDDetector_custom.cpp:298), because the reference's own
bitarray_custom.hpp includes <math.h>.  So the fixtures equal the oracle with PLI_PARITY_TRIG_F32_LBD = 1 and
PLI_PARITY_TRIG_F32_KEYLINE = 1, and differ from it with either flag clear (both defaults are 0 and stay 0).
"""
import collections
import os

import numpy as np
import pytest

import helpers_line_ref as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_EXE = os.path.join(ROOT, "oracle", "_ref", "pli_ref_line")
REF_EXE_MATHH = REF_EXE + "_mathh"
ids = lambda c: c.name


@pytest.fixture(scope="module")
def oracle():
    from oracle import pyoracle as po
    po.lib()
    return po


def _oracle_run(po, case, lbd_f32=True, keyline_f32=True):
    img = case.image()
    h, w = img.shape
    cfg = po.default_config(w, h, lsd_nfeatures=case.nfeatures, min_line_length=case.min_line_length)
    assert cfg.parity_flags == po.PARITY_TRIG_F32_ORB | po.PARITY_LSD_F64          # the defaults: both line flags clear
    cfg.parity_flags |= (po.PARITY_TRIG_F32_LBD if lbd_f32 else 0) | (po.PARITY_TRIG_F32_KEYLINE if keyline_f32 else 0)
    fr = po.Frame(cfg)
    if case.segments is None:
        n, kl, desc = fr.line_extract(0, img)
    else:
        n, kl, desc = fr.line_extract_from_segments(0, img, case.segments())
    dx, dy = fr.lbd_dxdy(0, (h, w))
    return {"kl": kl, "desc": desc, "fdesc": fr.lbd_float(0, n), "segs": fr.lsd_segments(0), "dx": dx, "dy": dy}


@pytest.fixture(scope="module")
def oracle_runs(oracle):
    """The oracle as this toolchain compiles the reference (both float overloads), once per case."""
    return {c.name: _oracle_run(oracle, c) for c in H.CASES}


def test_corpus_has_the_required_cases():
    names = [c.name for c in H.CASES]
    assert sorted(os.listdir(H.GOLD_DIR)) == sorted(n + ".npz" for n in names)
    assert sum(os.path.getsize(H.fixture_path(n)) for n in names) <= (1 << 20)
    shapes = {c.name: c.image().shape for c in H.IMAGE_CASES}
    assert all(h <= 240 and w <= 376 for h, w in shapes.values())
    assert any(h > w for h, w in shapes.values()) and any(w % 2 for h, w in shapes.values())
    assert len(H.SEGMENT_CASES) >= 8 and {len(c.segments()) for c in H.SEGMENT_CASES} >= {16, 17, 200}
    assert {c.min_line_length for c in H.IMAGE_CASES} >= {0.0, 0.025, 0.2}


@pytest.mark.parametrize("case", H.CASES, ids=ids)
def test_tie_groups_are_where_the_corpus_says(case):
    """Only the named tie cases hold equal responses at or before their cut, and they hold the groups they were built for."""
    H.check_tie_contract(case, H.load_fixture(case.name))


@pytest.mark.skipif(not (os.path.exists(REF_EXE) and os.path.exists(REF_EXE_MATHH)),
                    reason="oracle/_ref/pli_ref_line is built only where the reference tree exists")
@pytest.mark.parametrize("case", H.CASES, ids=ids)
def test_live_reference_equals_fixture(case):
    for exe, mathh in ((REF_EXE, False), (REF_EXE_MATHH, True)):
        fix = H.load_fixture(case.name, mathh=mathh)
        res = H.result_of_fixture_form(H.run_reference(exe, case), case)
        assert np.array_equal(res["segs"], fix["segs"]), (case.name, exe)
        assert res["kl"].tobytes() == fix["kl"].tobytes(), (case.name, exe, "key lines")
        assert res["desc"].tobytes() == fix["desc"].tobytes() and res["desc"].shape == fix["desc"].shape, (case.name, exe)
        assert res["fdesc"].tobytes() == fix["fdesc"].tobytes() and res["fdesc"].shape == fix["fdesc"].shape, (case.name, exe)
        assert (res["dx_sha"], res["dy_sha"], res["empty_message"]) == (fix["dx_sha"], fix["dy_sha"], fix["empty_message"]), (case.name, exe)
        if fix["dx"] is not None:
            assert np.array_equal(res["dx"], fix["dx"]) and np.array_equal(res["dy"], fix["dy"])


@pytest.mark.parametrize("case", H.CASES, ids=ids)
def test_oracle_equals_reference_fixture(oracle_runs, case):
    """Every key-line field, the 32 bytes, the 72 floats and both gradient planes, by bytes; rows in place except inside the tie groups
    of the named tie cases (helpers_line_ref.compare_with_ties)."""
    fix, got = H.load_fixture(case.name), oracle_runs[case.name]
    assert np.array_equal(got["segs"], fix["segs"]), "the detector stand-in and the oracle's detector returned different segments"
    msgs, moved_inside, moved_straddle = H.compare_with_ties(case, fix, got["kl"], got["desc"], got["fdesc"])
    print("%s: %d key lines, %d rows differ inside kept tie groups, %d from the straddling group on" % (
        case.name, len(fix["kl"]), moved_inside, moved_straddle))
    assert not msgs, (case.name, msgs)
    if case.name not in H.TIE_INSIDE + H.TIE_STRADDLE:
        assert got["kl"].tobytes() == fix["kl"].tobytes() and moved_inside == 0 and moved_straddle == 0
    if len(fix["kl"]):
        assert (H._sha(got["dx"]), H._sha(got["dy"])) == (fix["dx_sha"], fix["dy_sha"]), "gradient planes"
        if fix["dx"] is not None:
            assert np.array_equal(got["dx"], fix["dx"]) and np.array_equal(got["dy"], fix["dy"])
    else:
        # "Error: keypoint list is empty": computeSobel never ran and descriptors_line was left untouched
        assert fix["empty_message"] and fix["dx_sha"] is None and fix["desc"].shape == (0, 32) and got["desc"].shape == (0, 32)


def test_which_flag_value_each_binary_corresponds_to(oracle):
    """The two header regimes of the stand-in give the same bytes on every case: on this toolchain the overloads do not depend on it.
    The single flag value that equals them is 1, for PLI_PARITY_TRIG_F32_LBD (the 72 floats) and for PLI_PARITY_TRIG_F32_KEYLINE
    (KeyLine::angle); with either flag at its default 0 the oracle differs from the reference's bytes, in rows that are counted here."""
    assert all(H.load_fixture(c.name)["mathh_same"] for c in H.CASES)
    rows = floats_lbd0 = bytes_lbd0 = angle_kl0 = 0
    for c in H.CASES:
        if c.name in H.TIE_INSIDE + H.TIE_STRADDLE:
            continue
        fix = H.load_fixture(c.name)
        lbd0 = _oracle_run(oracle, c, lbd_f32=False)
        kl0 = _oracle_run(oracle, c, keyline_f32=False)
        assert lbd0["kl"].tobytes() == fix["kl"].tobytes()                      # the LBD flag does not reach the key lines
        for f in H.KEYLINE_DT.names:                                            # ... and the key-line flag reaches the angle only
            assert f == "angle" or kl0["kl"][f].tobytes() == fix["kl"][f].tobytes(), (c.name, f)
        rows += len(fix["kl"])
        floats_lbd0 += int((lbd0["fdesc"].view(np.int32) != fix["fdesc"].view(np.int32)).any(axis=1).sum())
        bytes_lbd0 += int((lbd0["desc"] != fix["desc"]).any(axis=1).sum())
        angle_kl0 += int((kl0["kl"]["angle"].view(np.int32) != fix["kl"]["angle"].view(np.int32)).sum())
        ulp = np.abs(kl0["kl"]["angle"].view(np.int32).astype(np.int64) - fix["kl"]["angle"].view(np.int32).astype(np.int64))
        assert ulp.max(initial=0) <= 1
    print("of %d rows: PLI_PARITY_TRIG_F32_LBD = 0 differs in the 72 floats of %d and the 32 bytes of %d; "
          "PLI_PARITY_TRIG_F32_KEYLINE = 0 differs in the angle of %d (by one ulp)" % (rows, floats_lbd0, bytes_lbd0, angle_kl0))
    assert floats_lbd0 > 0 and angle_kl0 > 0


def test_tie_order_report(oracle_runs):
    """libstdc++'s std::sort against the stable sort, on the tie cases: rows that differ inside kept tie groups and from a straddling
    group on.  The allowance stays because the order does differ (DESIGN.md holds the table this prints)."""
    moved = {}
    for name in H.TIE_INSIDE + H.TIE_STRADDLE:
        c, got = H.CASE_BY_NAME[name], oracle_runs[name]
        fix = H.load_fixture(name)
        _, mi, ms = H.compare_with_ties(c, fix, got["kl"], got["desc"], got["fdesc"])
        rows = lambda K: collections.Counter(b"".join(K[f][i:i + 1].tobytes() for f in H.FIELDS_WITHOUT_CLASS_ID) for i in range(len(K)))
        kept_differ = sum((rows(got["kl"]) - rows(fix["kl"])).values())
        moved[name] = (mi, ms, kept_differ)
        print("%-30s %3d lines kept: %3d rows differ inside kept groups, %3d from the straddling group on, %d kept lines are other lines" % (
            name, len(fix["kl"]), mi, ms, kept_differ))
    assert any(mi for mi, _, _ in moved.values()), "std::sort kept detection order everywhere: drop the tie allowance"
    for name in H.TIE_INSIDE:
        assert moved[name][1] == 0 and moved[name][2] == 0
    for name in H.TIE_SMALL:                                                      # <= 16 elements: insertion sort, in place (asserted above)
        assert len(H.before_cut(H.CASE_BY_NAME[name], H.load_fixture(name))[0]) <= 16


# ---------------------------------------------------------------------------------------------------------------- mutants
def _restated(case, planes, mut=None):
    fix = H.load_fixture(case.name)
    h, w = case.image().shape
    kl = H.restate_keylines(fix["segs"], w, h, case.nfeatures, case.min_line_length, mut)
    fdesc, desc = H.restate_lbd(kl, planes["dx"], planes["dy"], mut)
    return H.compare_with_ties(case, fix, kl, desc, fdesc)[0]


def test_python_restatement_equals_every_fixture(oracle_runs):
    for c in H.CASES:
        assert not _restated(c, oracle_runs[c.name]), c.name


@pytest.mark.parametrize("mut", H.MUTANTS)
def test_mutant_is_rejected(oracle_runs, mut):
    """One deliberate misreading at a time: the fixtures must tell it from the reading."""
    rejecting = [c.name for c in H.CASES if _restated(c, oracle_runs[c.name], mut)]
    print("%s: rejected by %d of %d cases" % (mut, len(rejecting), len(H.CASES)))
    assert rejecting, mut


# ------------------------------------------------------------------------------------------------------ branch accounting
def test_corpus_reaches_every_branch(oracle_runs):
    clamps = np.zeros(8, int)
    gate_kept = gate_dropped = gate_equal = cut_taken = cut_not_taken = empty = half_width_zero = collapsed = 0
    band = {}
    for c in H.CASES:
        fix = H.load_fixture(c.name)
        h, w = c.image().shape
        e, fired = H.clamp_segments(fix["segs"], w, h)
        clamps += fired.sum(axis=0)
        length = H.lengths_of(e).astype(np.float64)
        min_length = c.min_line_length * min(w, h)
        gate_kept += int((length > min_length).sum())
        gate_dropped += int((length <= min_length).sum())
        gate_equal += int(((length == min_length) & (min_length > 0)).sum())
        collapsed += int((fired.any(axis=1) & (length == 0)).sum())
        n_before = int((length > min_length).sum())
        taken = c.nfeatures != 0 and n_before > c.nfeatures
        cut_taken += taken
        cut_not_taken += not taken
        assert len(fix["kl"]) == (c.nfeatures if taken else n_before), c.name
        if taken:                                                                 # class_id re-numbered only when the cut happens
            assert fix["kl"]["class_id"].tolist() == list(range(c.nfeatures))
        empty += len(fix["kl"]) == 0 and fix["empty_message"]
        half_width_zero += int((fix["kl"]["numOfPixels"] <= 2).sum())
        if c.segments is None and len(fix["kl"]):
            H.restate_lbd(fix["kl"], oracle_runs[c.name]["dx"], oracle_runs[c.name]["dy"], cover=band)
    names = ("x1<0", "x1>=W", "x2<0", "x2>=W", "y1<0", "y1>=H", "y2<0", "y2>=H")
    print("clamps", dict(zip(names, clamps.tolist())), "gate kept/dropped/at min_length", gate_kept, gate_dropped, gate_equal,
          "cut taken/not", cut_taken, cut_not_taken, "band samples clamped (image cases)", band, "empty", empty, "numOfPixels<=2", half_width_zero)
    assert (clamps > 0).all(), dict(zip(names, clamps.tolist()))
    assert gate_kept and gate_dropped and gate_equal >= 2 and collapsed >= 2
    assert cut_taken >= 5 and cut_not_taken >= 5
    assert all(band.get(k, 0) > 0 for k in ("left", "right", "top", "bottom")), band
    assert empty == 1 and half_width_zero >= 1
    # lsd_nfeatures against the count before the cut: 0, larger, exactly the count, one under it, small
    rel = set()
    for c in H.IMAGE_CASES:
        n_before = len(H.before_cut(c, H.load_fixture(c.name))[0])
        rel.add("zero" if c.nfeatures == 0 else "larger" if c.nfeatures > n_before else "exact" if c.nfeatures == n_before else
                "minus1" if c.nfeatures == n_before - 1 else "small")
    assert rel == {"zero", "larger", "exact", "minus1", "small"}, rel
