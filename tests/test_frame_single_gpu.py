"""pli_frame_extract_single: the front-end of one monocular or RGB-D Frame of a distorted pinhole camera in one submission.

Against the separate calls on a second context — orb_extract_lapping(0, img, lapping) and line_extract(0, img) — the record's eye-0
columns are byte equal, with the lapping area of the monocular constructor ({0, 1000}: every keypoint on the lapping side, the table
reversed) and of the RGB-D one ({0, 0}); kp_un, cell and kl_un equal the float64 restatement (tests/helpers_undistort.py) applied to
those keypoints and keylines; uright and depth equal its restatement of Frame.cc:1309-1330 on a constructed depth image (a plane
with a band of zeros and a band of negative values), which is read at the DISTORTED keypoint while mvuRight takes the UNDISTORTED
x.  320 x 240 context, the TUM-like camera scaled by 0.5, a photograph and a synthetic image."""
import ctypes as C

import numpy as np
import pytest

import helpers_undistort as hu

pytestmark = pytest.mark.gpu

W, H = 320, 240
CAM = hu.scaled(hu.TUM[0], 0.5)
MONO, RGBD = (0, 1000), (0, 0)          # Frame.cc:360, :258


def _images():
    from pli_slam_amd import realdata, synth
    return {"photo": realdata.frames_752x480(1, seed=3, w=W, h=H)[0][0], "synth": synth.make_stereo_pair(12, W, H)[0]}


def _depth():
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
    d = (np.float32(1.5) + np.float32(0.004) * xs + np.float32(0.002) * ys).astype(np.float32)
    d[70:100] = 0
    d[150:175] = np.float32(-2.5)
    return d


@pytest.fixture(scope="module")
def ctx():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from pli_slam_amd import capi
    from pli_slam_amd.frontend import Frontend
    cfg = capi.default_config(W, H, orb_nfeatures=300, lsd_nfeatures=50)
    one, sep = Frontend(cfg), Frontend(cfg)
    bounds = one.set_pinhole_distortion(CAM)
    assert bounds.tobytes() == hu.image_bounds(CAM, W, H).tobytes()
    imgs = _images()
    # the separate calls, once per image and lapping area: (n, mono, kp, desc, m, kl, ldesc)
    want = {}
    for name, img in imgs.items():
        for lap in (MONO, RGBD):
            n, mono, kp, desc = sep.orb_extract_lapping(0, img, lap)
            m, kl, ld = sep.line_extract(0, img)
            want[name, lap] = (n, mono, kp, desc, m, kl, ld)
    yield dict(capi=capi, cfg=cfg, one=one, sep=sep, imgs=imgs, want=want, bounds=bounds, depth=_depth())
    one.close()
    sep.close()


def _xy(kp):
    return np.stack([kp["x"], kp["y"]], axis=1).astype(np.float32)


def _check_columns(ctx, rec, name, lap):
    n, mono, kp, desc, m, kl, ld = ctx["want"][name, lap]
    assert n > 50 and m > 5, (n, m)
    assert rec["counts"][0] == n and rec["counts"][2] == m and not rec["truncated"][[0, 2]].any()
    assert rec["kpL"].tobytes() == kp.tobytes() and rec["descL"].tobytes() == desc.tobytes()
    assert rec["klL"].tobytes() == kl.tobytes() and rec["ldescL"].tobytes() == ld.tobytes()
    assert rec["n_mono"] == mono
    un = hu.undistort_points(_xy(kp), CAM)
    assert rec["kp_un"].tobytes() == un.tobytes()
    assert rec["cell"].tobytes() == hu.pos_in_grid(un, ctx["bounds"]).tobytes()
    s = hu.undistort_points(np.stack([kl["startPointX"], kl["startPointY"]], axis=1), CAM)
    e = hu.undistort_points(np.stack([kl["endPointX"], kl["endPointY"]], axis=1), CAM)
    assert rec["kl_un"].tobytes() == np.concatenate([s, e], axis=1).astype(np.float32).tobytes()
    # rows from the counts on: 0 / -1
    full = rec["full"]
    assert not full["kp_un"][n:].any() and not full["kl_un"][m:].any() and (full["cell"][n:] == -1).all()
    return kp, un


@pytest.mark.parametrize("name", ["photo", "synth"])
def test_monocular_frame_equals_the_separate_calls_and_the_restatement(ctx, name):
    img = ctx["imgs"][name]
    rec = ctx["one"].frame_extract_single(img, MONO)
    kp, _ = _check_columns(ctx, rec, name, MONO)
    # {0, 1000}: every keypoint is on the lapping side, so the table is the extractor's in reverse and monoLeft is 0
    n0, kp0, _ = ctx["sep"].orb_extract(0, img)
    assert rec["n_mono"] == 0 and n0 == len(kp) and kp.tobytes() == kp0[::-1].tobytes()
    # no depth image: mvuRight = mvDepth = -1 in every row (Frame.cc:384-385)
    Y = ctx["one"].layout
    raw = rec["full"]["record"]
    for off in (Y.off_uright, Y.off_depth):
        assert (raw[off:off + 4 * ctx["one"].kp_cap].view(np.float32) == -1).all()
    assert (rec["uright"] == -1).all() and (rec["depth"] == -1).all()


@pytest.mark.parametrize("name", ["photo", "synth"])
def test_rgbd_frame_reads_depth_at_the_distorted_keypoint(ctx, name):
    img, depth = ctx["imgs"][name], ctx["depth"]
    rec = ctx["one"].frame_extract_single(img, RGBD, depth)
    kp, un = _check_columns(ctx, rec, name, RGBD)
    assert rec["n_mono"] == len(kp)                        # {0, 0}: no keypoint has x == 0, none is on the lapping side
    want_ur, want_dp = hu.stereo_from_rgbd(_xy(kp), un, depth, ctx["cfg"].bf)
    assert rec["uright"].tobytes() == want_ur.tobytes() and rec["depth"].tobytes() == want_dp.tobytes()
    d = depth[kp["y"].astype(np.int32), kp["x"].astype(np.int32)]
    assert (d > 0).any() and (d == 0).any() and (d < 0).any()                   # both branches of :1324
    assert (want_dp[d > 0] == d[d > 0]).all() and (want_dp[d <= 0] == -1).all()
    # a depth read at the undistorted position, or mvuRight from the distorted x, would show
    moved = kp["x"].astype(np.int32) != un[:, 0].astype(np.int32)
    assert moved.any() and (d > 0)[moved].any()
    wrong_ur, wrong_dp = hu.stereo_from_rgbd(un, un, depth, ctx["cfg"].bf)
    assert wrong_dp.tobytes() != want_dp.tobytes()
    assert hu.stereo_from_rgbd(_xy(kp), _xy(kp), depth, ctx["cfg"].bf)[0].tobytes() != want_ur.tobytes()
    # a depth image with padded rows is the same call
    padded = np.full((H, W + 8), np.float32(9.75), np.float32)
    padded[:, :W] = depth
    rec2 = ctx["one"].frame_extract_single(img, RGBD, padded)
    assert rec2["uright"].tobytes() == want_ur.tobytes() and rec2["depth"].tobytes() == want_dp.tobytes()


def test_twice_gives_identical_bytes_and_the_state_left_behind_serves_the_per_call_entry_points(ctx):
    one, sep, capi = ctx["one"], ctx["sep"], ctx["capi"]
    img, depth = ctx["imgs"]["photo"], ctx["depth"]
    a = one.frame_extract_single(img, RGBD, depth)
    one.frame_extract_single(ctx["imgs"]["synth"], MONO)                        # another Frame in between
    b = one.frame_extract_single(img, RGBD, depth)
    for k in ("record", "kp_un", "kl_un", "cell"):
        assert a["full"][k].tobytes() == b["full"][k].tobytes(), k
    assert a["n_mono"] == b["n_mono"]
    n, mono, kp, desc, m, kl, ld = ctx["want"]["photo", RGBD]
    counts = (C.c_int32 * 4)()
    capi.check(one.L.pli_last_counts(one.h, counts))
    assert counts[0] == n and counts[2] == m
    # the pyramid of this Frame ...
    sep.orb_extract(0, img)
    assert np.array_equal(one.pyramid_level(0, 0), img)
    for level in (1, 3):
        assert np.array_equal(one.pyramid_level(0, level), sep.pyramid_level(0, level))
    # ... and its keypoint table: the existing RGB-D association (rectified pipeline: it takes the keypoint's own x) runs on it
    ur, dp = one.stereo_from_depth(depth)
    want_ur, want_dp = hu.stereo_from_rgbd(_xy(kp), _xy(kp), depth, ctx["cfg"].bf)
    assert ur[:n].tobytes() == want_ur.tobytes() and dp[:n].tobytes() == want_dp.tobytes()


def test_without_a_camera_the_undistorted_columns_are_copies(ctx):
    one = ctx["one"]
    img = ctx["imgs"]["synth"]
    one.set_pinhole_distortion(None)
    try:
        rec = one.frame_extract_single(img, RGBD, ctx["depth"])
    finally:
        one.set_pinhole_distortion(CAM)
    n, mono, kp, desc, m, kl, ld = ctx["want"]["synth", RGBD]
    assert rec["kpL"].tobytes() == kp.tobytes()
    assert rec["kp_un"].tobytes() == _xy(kp).tobytes()
    assert rec["cell"].tobytes() == hu.pos_in_grid(_xy(kp), np.array([0, W, 0, H], np.float32)).tobytes()
    ends = np.stack([kl["startPointX"], kl["startPointY"], kl["endPointX"], kl["endPointY"]], axis=1).astype(np.float32)
    assert rec["kl_un"].tobytes() == ends.tobytes()
    want_ur, want_dp = hu.stereo_from_rgbd(_xy(kp), _xy(kp), ctx["depth"], ctx["cfg"].bf)
    assert rec["uright"].tobytes() == want_ur.tobytes() and rec["depth"].tobytes() == want_dp.tobytes()


def test_bad_arguments_are_errors(ctx):
    one, capi = ctx["one"], ctx["capi"]
    with pytest.raises(capi.PliError):
        one.frame_extract_single(np.zeros((H + 1, W), np.uint8), MONO)
    img = ctx["imgs"]["synth"]
    mono = C.c_int32()
    assert one.L.pli_frame_extract_single(one.h, capi.ptr(img), W, H, W, 0, 0, None, 0, None, None, None, None, C.byref(mono)) == -1
    assert one.L.pli_undistort_points(one.h, None, 3, None, None) == -1
