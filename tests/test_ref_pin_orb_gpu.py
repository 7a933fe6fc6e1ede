"""The device's ORB chain against the reference's own recorded outputs (tests/golden/orb_ref, see tests/test_ref_pin_orb.py and
tests/helpers_orb_ref.py), not against the oracle: pyramid, per-cell FAST, DistributeOctTree, IC_Angle, steered BRIEF, the rescale
to level 0 and the lapping order, through Frontend.orb_extract, orb_extract_lapping, pyramid_level and, as frame 1 of a two-frame
batch whose frame 0 is a different image, batch_run_host.  Byte equality over every row of every case; no tolerance.
Reads only the fixtures and the helper.
"""
import numpy as np
import pytest

import helpers_orb_ref as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from pli_slam_amd import capi
    from pli_slam_amd.frontend import Frontend
    return capi, Frontend


def _lapping_order(kp, lap):
    """ORBextractor.cc:1135-1144 on a level-major table: lap0 <= x <= lap1 fills the table from the back, the rest from the front."""
    x = kp["x"]
    tail = (x >= np.float32(lap[0])) & (x <= np.float32(lap[1]))
    idx = np.arange(len(kp))
    return np.concatenate([idx[~tail], idx[tail][::-1]]), int((~tail).sum())


def _assert_rows_equal(kp, desc, fix, what):
    assert len(kp) == len(fix["kp"]), (what, "keypoint count", len(kp), len(fix["kp"]))
    for f in kp.dtype.names:
        d = np.flatnonzero(kp[f].view(np.int32) != fix["kp"][f].view(np.int32))
        assert d.size == 0, "%s: kp.%s differs from the reference's at rows %s (%d rows)" % (what, f, d[:5], d.size)
    assert kp.tobytes() == fix["kp"].tobytes(), what
    d = np.flatnonzero((desc != fix["desc"]).any(axis=1))
    assert d.size == 0, "%s: descriptors differ from the reference's at rows %s (%d rows)" % (what, d[:5], d.size)


@pytest.mark.parametrize("group", H.groups(), ids=lambda g: "%dx%d_n%d_f%g_l%d_th%d_%d" % g[0])
def test_device_equals_reference_fixture(gpu, group):
    capi, Frontend = gpu
    p, cases = group
    cfg = capi.default_config(p.W, p.H, orb_nfeatures=p.nfeatures, orb_scale_factor=p.scale_factor, orb_nlevels=p.nlevels,
                              orb_ini_th_fast=p.ini_th, orb_min_th_fast=p.min_th, lsd_nfeatures=20, max_frames=2)
    fe = Frontend(cfg)
    images = [c.image() for c in cases]
    for i, (c, img) in enumerate(zip(cases, images)):
        fix = H.load_fixture(c.name)
        eye = i % 2
        n, mono, kp, desc = fe.orb_extract_lapping(eye, img, c.lapping)
        assert n == len(fix["kp"]) and mono == fix["mono"], (c.name, n, mono, fix["mono"])
        _assert_rows_equal(kp, desc, fix, c.name + " orb_extract_lapping")
        if c.pyramid:
            for l, ref in enumerate(fix["levels"]):
                got = fe.pyramid_level(eye, l)
                assert got.shape == ref.shape and np.array_equal(got, ref), (c.name, "pyramid level", l)
        # the plain entry points return the level-major table; put into the lapping order here, it is the reference's table
        n2, kp2, desc2 = fe.orb_extract(1 - eye, img)
        order, mono2 = _lapping_order(kp2, c.lapping)
        assert n2 == len(fix["kp"]) and mono2 == fix["mono"]
        _assert_rows_equal(kp2[order], desc2[order], fix, c.name + " orb_extract")
        if c.lapping == (0, 0):
            _assert_rows_equal(kp2, desc2, fix, c.name + " orb_extract, table as returned")
        other = images[(i + 1) % len(images)] if len(images) > 1 else np.ascontiguousarray(img[::-1, ::-1])
        assert not np.array_equal(other, img)
        recs = fe.batch_run_host(np.stack([np.stack([other, other]), np.stack([img, other])]), stages=capi.RUN_ORB)
        kp3, desc3 = recs[1]["kpL"], recs[1]["descL"]
        order, mono3 = _lapping_order(kp3, c.lapping)
        assert mono3 == fix["mono"]
        _assert_rows_equal(kp3[order], desc3[order], fix, c.name + " batch_run_host frame 1")
        assert recs[1]["kpR"].tobytes() == recs[0]["kpL"].tobytes() and np.array_equal(recs[1]["descR"], recs[0]["descL"])
    fe.close()
