"""The development build's other widths of the grid-cell searches: k_fuse_match with 16 and 64 lanes per surviving pair
(PLI_FUSE_LANES; the product runs 8) and the candidate lists of pli_search_by_projection_sim3 / _reloc with 1 and 64 keys
(PLI_SIM3_WIDTH; the product runs 16).  The product tests run none of them, and they are instantiations of the same templated device
code.  Equality with the Python restatements of tests/test_fuse_search_cpu.py, test_sim3_projection_cpu.py and
test_reloc_projection_cpu.py is exact, as in the product tests.

One scene for all of them: 8 spots on the corners of grid cells, two keypoints beside every spot (one within half a pixel, with the spot's
descriptor a few bits away, one within 1.5 px, with a random descriptor), 40 copies of each within +-2.5 px: 640 rows.  60 points lie on the spots,
several on each.  So a window holds about 80 rows - more than a 64-lane group takes in one step - in four cells, of which the 40
near copies are within the limits: more than a list of 1 holds (every contested window takes the overflow path of the ordered walk),
fewer than a list of 64 holds (none does).  The switches are read per call, so they are set and restored around each call."""
import contextlib
import os

import numpy as np
import pytest

from pli_slam_amd import capi
from test_fuse_search_cpu import (CAM, IDENTITY, KF, NLEVELS, SF, flip_bits, fuse_search_fast, fuse_search_scalar, level_ratio,
                                  one_point)
from test_reloc_projection_cpu import FR, Cand, reloc_search_fast, wrap360
from test_sim3_projection_cpu import sim3_search_fast

W, H = 752, 480
NSPOT, REP, NPTS = 8, 40, 60


def scene():
    """-> points[60], descs, crowded KF of 640 rows, the spot of every point"""
    rng = np.random.default_rng(21)
    f32 = np.float32
    spots, sdesc, xs, ys, octs, ds, urs = [], rng.integers(0, 256, (NSPOT, 32), dtype=np.uint8), [], [], [], [], []
    for s in range(NSPOT):
        # PosInGrid rounds: (k + 0.5) * 11.75 and (m + 0.5) * 10 are the borders between cell columns / rows
        u, v, z = (5 + 7 * s + 0.5) * 11.75, (4 + 5 * s + 0.5) * 10.0, float(rng.uniform(3.0, 12.0))
        lev = s % 4                                                  # radius th * 1.2^lev: 3 px at the least
        pos = np.array([(u - float(CAM.cx)) * z / float(CAM.fx), (v - float(CAM.cy)) * z / float(CAM.fy), z])
        spots.append(one_point(pos, max_dist=np.linalg.norm(pos) * float(SF[lev]) * 0.95))     # PredictScale gives lev
        for near in (True, False):
            off = 0.5 if near else 1.5
            kx, ky = u + rng.uniform(-off, off), v + rng.uniform(-off, off)
            for _ in range(REP):
                x, y = kx + rng.uniform(-2.5, 2.5), ky + rng.uniform(-2.5, 2.5)
                xs.append(x); ys.append(y)
                octs.append(int(np.clip(lev + rng.choice([0, 0, -1, 1]), 0, NLEVELS - 1)))
                ds.append(flip_bits(rng, sdesc[s], int(rng.choice([0, 3, 10]))) if near else rng.integers(0, 256, 32, dtype=np.uint8))
                urs.append(x - float(CAM.bf) / z + rng.normal(0, 0.5) if rng.random() < 0.6 else -1.0)
    order = rng.permutation(len(xs))
    kf = KF(np.array(xs, f32)[order], np.array(ys, f32)[order], np.array(octs, np.int32)[order],
            np.array(ds, np.uint8).reshape(-1, 32)[order], np.array(urs, f32)[order], IDENTITY)
    pick = rng.integers(0, NSPOT, NPTS)
    return np.concatenate(spots)[pick], sdesc[pick], kf, pick


PTS, DESCS, CROWDED, PICK = scene()
SAME = CROWDED._replace(desc=np.zeros_like(CROWDED.desc))            # all descriptors equal: the visiting order decides every winner
FUSE_CASES = [(3.0, True), (4.0, False)]                             # th, the chi-square gate
SIM3_CASES = [(3.0, 1.0, 0), (8.0, 1.5, 1)]                          # th, ratio, projection form
RELOC_CASES = [(10.0, 100, True), (3.0, 64, False)]                  # th, ORBdist (Tracking.cc:4290, :4304), the rotation filter
ANGLES = wrap360(np.random.default_rng(22).uniform(0, 360, NPTS + len(CROWDED.x)))
FRAME = FR(CROWDED.x, CROWDED.y, CROWDED.octave, CROWDED.desc, ANGLES[NPTS:])
CAND = Cand(PTS, DESCS, ANGLES[:NPTS], IDENTITY, None)


def test_the_scene_crowds_its_windows_and_matches():
    """On the CPU: what makes the equalities below say something."""
    assert len(CROWDED.x) == 640 and len(PTS) == NPTS
    for kf, descs in ((CROWDED, DESCS), (SAME, np.zeros_like(DESCS))):
        for th, gate in FUSE_CASES:
            info = {}
            bi, bd = fuse_search_fast(PTS, descs, kf, CAM, th, gate, info=info)
            # the restatement for this seed: each of the 60 windows holds 71 to 80 rows at th 3 and all 80 at th 4, and all 60
            # points match in the four settings; floors = every window above a lane group, half of the matches
            assert (info["window_rows"] > 64).all(), info["window_rows"]
            assert (bi >= 0).sum() > 30
    for th, ratio, form in SIM3_CASES:
        info = {}
        _, bi, nm = sim3_search_fast(PTS, DESCS, CROWDED, CAM, th, ratio, form, info=info)
        # for this seed: 60 lists of 26 to 35 keys, 60 matches; floors = every list between the two widths, half of the matches
        assert info["listed"].min() > 1 and info["listed"].max() <= 64 and nm > 30
    for th, orb_dist, ori in RELOC_CASES:
        info = {}
        _, bi, nm = reloc_search_fast(CAND, FRAME, CAM, th, orb_dist, ori, info=info)
        # for this seed: 60 lists of 40 keys; 60 matches without the rotation filter, 21 with it; floors = half of the matches
        assert info["listed"].min() > 1 and info["listed"].max() <= 64 and nm > (10 if ori else 30)


@pytest.fixture(scope="module")
def fe():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from pli_slam_amd.frontend import Frontend
    f = Frontend(capi.default_config(W, H), dev=True)
    assert f.dev and f.L is capi.lib(dev=True)                       # the build that reads the switches: the results cannot tell
    assert np.array_equal(f.cfg.orb_nlevels, NLEVELS)
    yield f
    f.close()


@contextlib.contextmanager
def switch(name, value):
    old = os.environ.get(name)
    os.environ[name] = str(value)
    try:
        yield
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


def keypoints(t, angle=None):
    kp = np.zeros(len(t.x), capi.KEYPOINT_DT)
    kp["x"], kp["y"], kp["octave"], kp["size"] = t.x, t.y, t.octave, 31.0
    if angle is not None:
        kp["angle"] = angle
    return kp


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [16, 64])
def test_fuse_search_with_other_lane_groups(fe, lanes):
    for kf, descs in ((CROWDED, DESCS), (SAME, np.zeros_like(DESCS))):
        for th, gate in FUSE_CASES:
            with switch("PLI_FUSE_LANES", lanes):
                bi, bd = fe.fuse_search(PTS, descs, [(keypoints(kf), kf.desc, kf.uright, kf.pose)], CAM, th, gate, None,
                                        level_ratio=level_ratio())
            # (the reference's control flow where the visiting order and the gate decide together, the closed form elsewhere)
            wi, wd = (fuse_search_scalar if kf is SAME and gate else fuse_search_fast)(PTS, descs, kf, CAM, th, gate)
            assert np.array_equal(bi[0], wi), "%d of %d best_idx differ" % (int((bi[0] != wi).sum()), wi.size)
            assert np.array_equal(bd[0], wd), "%d of %d best_dist differ" % (int((bd[0] != wd).sum()), wd.size)


@pytest.mark.gpu
@pytest.mark.parametrize("width", [1, 64])
def test_sim3_projection_with_other_list_widths(fe, width):
    for th, ratio, form in SIM3_CASES:
        with switch("PLI_SIM3_WIDTH", width):
            rows, bi, nm = fe.search_by_projection_sim3(PTS, DESCS, [(keypoints(CROWDED), CROWDED.desc, CROWDED.pose, None)], CAM, th,
                                                        ratio, form, None, level_ratio=level_ratio())
        wr, wi, wn = sim3_search_fast(PTS, DESCS, CROWDED, CAM, th, ratio, form)
        assert np.array_equal(bi[0], wi), "%d of %d best_idx differ" % (int((bi[0] != wi).sum()), wi.size)
        assert np.array_equal(rows[0], wr) and nm[0] == wn


@pytest.mark.gpu
@pytest.mark.parametrize("width", [1, 64])
def test_reloc_projection_with_other_list_widths(fe, width):
    for th, orb_dist, ori in RELOC_CASES:
        with switch("PLI_SIM3_WIDTH", width):
            rows, bi, nm = fe.search_by_projection_reloc([tuple(CAND)], keypoints(FRAME, FRAME.angle), FRAME.desc, CAM, th, orb_dist, ori,
                                                         level_ratio=level_ratio())
        wr, wi, wn = reloc_search_fast(CAND, FRAME, CAM, th, orb_dist, ori)
        assert np.array_equal(bi[0], wi), "%d of %d best_idx differ" % (int((bi[0] != wi).sum()), wi.size)
        assert np.array_equal(rows[0], wr) and nm[0] == wn
