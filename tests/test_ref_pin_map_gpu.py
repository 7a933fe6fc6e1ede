"""pli_search_local_points, pli_search_local_lines, pli_distinctive_descriptors, pli_create_new_map_points and pli_create_new_map_points_two_cameras on the MI355X (the
product library) against the answers of the reference's own compiled code recorded in tests/golden/map_ref
(tests/helpers_map_ref.py; tests/test_ref_pin_map.py holds the restatements to the same fixtures on the CPU).  Equality is exact,
as in tests/test_local_map_gpu.py, tests/test_distinctive_gpu.py and tests/test_new_map_points_gpu.py, but for the x3D of the
two-camera form, which is held to the bound of its helper (a NaN is compared as a NaN:
helpers_local_map.canonical).  Reads only the fixtures and the helper."""
import numpy as np
import pytest

import helpers_map_ref as H
from pli_slam_amd import capi

pytestmark = pytest.mark.gpu
ids = lambda c: c.name


@pytest.fixture(scope="module")
def fe():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from pli_slam_amd.frontend import Frontend
    f = Frontend(capi.default_config(752, 480), dev=False)
    yield f
    f.close()


@pytest.mark.parametrize("case", H.BY_FN["frustum_points"], ids=ids)
def test_local_points_equal_the_reference(fe, case):
    a, res = H.load_fixture(case.name)
    want = case.expected(a, res)
    got = case.device(fe, a)
    assert case.same(want, got), (case.name, "records differ at", [i for i in range(len(want[0])) if H.lm.canonical(want[0][i:i + 1]) !=
                                  H.lm.canonical(got[0][i:i + 1])][:8], "best_idx2 at", np.flatnonzero(want[1] != got[1])[:8], want[2:], got[2:])


@pytest.mark.parametrize("case", H.BY_FN["frustum_lines"], ids=ids)
def test_local_lines_equal_the_reference(fe, case):
    a, res = H.load_fixture(case.name)
    want = case.expected(a, res)
    got, (m, n) = case.device(fe, a)
    assert case.same(want, got), (case.name, want[0].tolist(), got[0].tolist(), want[2].tolist(), got[2].tolist())
    # the match of Tracking.cc:3882 on the PINNED list: matchNNR, which the stereo pin holds to the reference
    lst = want[2]
    wn, wm = H.hm.match_nnr(a["ml_desc"][lst], a["cur_desc"], float(a["params"][0])) if len(lst) else (0, np.zeros(0, np.int32))
    assert m.tobytes() == np.asarray(wm, np.int32).tobytes() and n == wn, case.name


@pytest.mark.parametrize("case", H.BY_FN["distinctive"], ids=ids)
def test_distinctive_descriptors_equal_the_reference(fe, case):
    a, res = H.load_fixture(case.name)
    want = case.expected(a, res)
    got = case.device(fe, a)
    assert case.same(want, got), (case.name, None if want[0] is None else np.flatnonzero(want[0] != got[0])[:8], np.flatnonzero(want[1] != got[1])[:8])


@pytest.mark.parametrize("case", H.BY_FN["new_map_points"], ids=ids)
def test_new_map_points_equal_the_reference(fe, case):
    """matches12 as the loop saw them, which pairs became map points, the bits of x3D and the creation sequence (the enumeration
    neighbours in order, idx1 ascending, status == CREATED): exact, as tests/test_new_map_points_gpu.py is against its restatement.
    Once with all neighbours in one call, once per neighbour, chained through has_mp by hand."""
    a, res = H.load_fixture(case.name)
    want = case.expected(a, res)
    for chained in (False, True):
        got = case.device(fe, a, chained)
        assert case.same(want, got), (case.name, "chained" if chained else "one call", np.argwhere(want[0] != got[0])[:5],
                                      np.argwhere(want[1] != got[1])[:5])


@pytest.mark.parametrize("case", H.BY_FN["new_map_points_two_cameras"], ids=ids)
def test_new_map_points_two_cameras_equal_the_reference(fe, case):
    """The mpCamera2 branch: vMatchedIndices, the created pairs and the creation sequence exactly; x3D to the bound
    helpers_new_map_points_two_cameras.MEASURED["x3d_rel"] (TwoCamerasCase.same: the reference's unprojection goes through the C
    library).  All neighbours in one call, and one call per neighbour chained through has_mp by hand."""
    a, res = H.load_fixture(case.name)
    want = case.expected(a, res)
    for chained in (False, True):
        got = case.device(fe, a, chained)
        assert case.same(want, got), (case.name, "chained" if chained else "one call", np.argwhere(want[0] != got[0])[:5],
                                      np.argwhere(want[1] != got[1])[:5])
        print(case.name, "x3D bit for bit: %d of %d" % case.bit_equal(want, got))
