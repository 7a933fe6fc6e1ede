"""k_fisheye_triangulate (through pli_stereo_fisheye_tables) against the reference's own recorded answers
(tests/golden/match_ref_two_cameras, see tests/test_ref_pin_match_two_cameras.py and tests/helpers_match_ref_two_cameras.py), not
against the oracle: the keypoint pairs of every kb8 case go through the device as two tables whose left row i and right row i share
one descriptor at Hamming distance >= 128 from every other row, so the matching stage can only pair row i with row i, and depth and
p3d must equal what the compiled KannalaBrandt8::TriangulateMatches returned, bit for bit, -1 and zeros for a rejected pair.

The one residue: where the reference's tanf, in one of the pair's two unprojections, returned a float next to the
correctly rounded value (helpers: tri_residue finds these pairs from the recorded rays, in float64), the device, which rounds
correctly, may differ; such a pair is still accepted or rejected alike and lies within twice the float64 envelope of
helpers_geometry.  No other pair may differ.  Reads only the fixtures and the helper.
"""
import numpy as np
import pytest

import helpers_geometry as G
import helpers_match_ref_two_cameras as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fe():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from pli_slam_amd import capi
    from pli_slam_amd.frontend import Frontend
    f = Frontend(capi.default_config(512, 512, orb_nfeatures=500, lsd_nfeatures=0))
    assert f.cfg.orb_nlevels == len(G.fisheye_sigma2())                    # mvLevelSigma2 of the device is the helper's
    yield f
    f.close()


@pytest.mark.parametrize("case", H.KB8_CASES, ids=lambda c: c.name)
def test_device_triangulation_equals_reference_fixture(fe, case):
    a, res = H.load_fixture(case.name)
    kpL, dL, kpR, dR = case.tables(a)
    assert len(kpL) <= H.MAX_ROWS // 2
    n, l2r, r2l, depth, p3d = fe.stereo_fisheye_tables(kpL, dL, 0, kpR, dR, 0, a["cam1"], a["cam2"], a["R12"], a["t12"])
    want_depth, want_p3d = H.tri_expected(res["call"])
    residue = H.tri_residue(a, res["call"])
    ok = want_depth > 0
    assert n == int(ok.sum()) and np.array_equal(depth > 0, ok), case.name
    assert np.array_equal(l2r, np.where(ok, np.arange(len(ok)), -1)) and np.array_equal(r2l, l2r), case.name
    assert np.all(depth[~ok] == np.float32(-1)) and not p3d[~ok].any(), case.name
    differs = (depth.view(np.uint32) != want_depth.view(np.uint32)) | (p3d.view(np.uint32) != want_p3d.view(np.uint32)).any(1)
    print("%s: %d of %d pairs at a tanf residue input, %d of them differ" % (case.name, residue.sum(), len(ok), differs.sum()))
    assert not np.any(differs & ~residue), (case.name, np.nonzero(differs & ~residue)[0])
    tn = float(np.linalg.norm(a["t12"].astype(np.float64)))
    z = want_depth.astype(np.float64)
    tol = 2 * G.FISHEYE_TOL_C[case.tol] * G.EPS32 * np.maximum(1.0, z * z / tn)
    assert np.all(np.abs(depth.astype(np.float64) - want_depth) <= tol), case.name
    assert np.all(np.abs(p3d.astype(np.float64) - want_p3d) <= tol[:, None]), case.name


@pytest.mark.parametrize("case", H.TRI2_CASES + H.BOW2_CASES + H.FUSE2_CASES + H.LOCAL2_CASES + H.FRAME2_CASES, ids=lambda c: c.name)
def test_device_search_equals_reference_fixture(fe, case):
    """search_for_triangulation_two_cameras (bOnlyStereo, bCoarse, mbCheckOrientation all ways), search_by_bow_two_cameras,
    fuse_search_two_cameras (sides 3, and 1 / 2 alone) and search_local_map_fisheye / search_by_projection_two_cameras (one frame: one call), once with every neighbour / keyframe / side of the case in ONE call and once
    per reference call: both equal what the reference's SearchForTriangulation / SearchByBoW(pKF, F, ...) / Fuse(pKF, vpMapPoints,
    th, bRight) returned, exactly (for Fuse: the rows found and the calls on the map that follow from them, in order)."""
    a, results = H.load_fixture(case.name)
    got = case.device(fe, a, case.calls)
    assert sorted(got) == sorted(case.calls)
    for call in case.calls:
        want = case.expected(a, call, results[call])
        batched, single = got[call]
        assert H.same(want, single), (case.name, call, "a call of its own")
        assert H.same(want, batched), (case.name, call, "one call over the whole case")
