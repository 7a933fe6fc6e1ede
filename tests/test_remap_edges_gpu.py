"""Edges of two small device paths that were held to the oracle at one ordinary shape each.

The rectification remap fused into k_ingest: level 0 against oracle.remap_linear, byte equal, at a width that is and one that is
not a multiple of the four pixels a thread stores, with map entries planted at the image border, far outside it, beyond the range
of an int after the multiplication by 32, infinite and NaN.  (What oracle.remap_linear itself computes is held to a plain bilinear
interpolation in tests/test_independent_checks.py.)  cv::remap converts with cvRound, which on x86 answers INT_MIN for a NaN and
for a value that does not fit an int; INT_MIN lies outside every image, so such a pixel takes the border value 0.

The RGB-D association k_stereo_from_depth: against five lines of numpy written from Frame.cc:1309-1331, on the call's own
keypoints, with the depth cells under the keypoints holding 0, -0.0, a negative value, NaN, +inf, the smallest denormal, 1e-30, bf
itself and ordinary depths; through the wrapper, and through a padded buffer with a row stride larger than the width.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from oracle import pyoracle as po
    from pli_slam_amd import capi
    from pli_slam_amd.frontend import Frontend
    return capi, Frontend, po


def _planted_maps(W, H):
    """A gentle warp, with single entries replaced, one axis at a time (the other axis stays inside the image).
    -> (mapx, mapy, [(x, y, axis, value)])."""
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
    mx = (xs + np.float32(0.3) + np.float32(0.01) * ys).astype(np.float32)
    my = (ys - np.float32(0.2) + np.float32(0.005) * xs).astype(np.float32)
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    planted = []
    for axis, size, row0 in ((0, W, 4), (1, H, 50)):
        values = [-0.5, -1.0, -1.03, size - 1, size - 0.5, size, 40000, 7e7, -7e7, 1e9, -1e9, inf, -inf, nan]
        for i, v in enumerate(values):
            planted.append(((7 * i + 3) % W, row0 + 3 * i, axis, np.float32(v)))
        # the non-finite ones again in the last four columns (the thread that stores past a width that is no multiple of 4) and
        # in column 0
        for j, v in enumerate((nan, inf, -inf, nan)):
            planted.append((W - 1 - j, row0 + 1 + 3 * j, axis, v))
        planted.append((0, row0 + 2, axis, nan))
    assert len({(x, y) for x, y, _, _ in planted}) == len(planted) and all(0 <= y < H for _, y, _, _ in planted)
    for x, y, axis, v in planted:
        (mx if axis == 0 else my)[y, x] = v
    return mx, my, planted


def _assert_level0(got, want, mx, my, planted, what):
    H, W = want.shape
    got = got.reshape(H, W)
    bad = np.argwhere(got != want)
    report = [(int(x), int(y), int(got[y, x]), int(want[y, x]), float(mx[y, x]), float(my[y, x])) for y, x in bad[:8]]
    assert not len(bad), "%s: %d pixels differ from the oracle's remap; (x, y, device, oracle, mapx, mapy): %s" % (what, len(bad), report)


@pytest.mark.parametrize("W,H", [(128, 96), (131, 97)])
def test_remap_border_far_and_non_finite_map_entries(gpu, W, H):
    capi, Frontend, po = gpu
    rng = np.random.default_rng(W)
    img = rng.integers(16, 256, (H, W), dtype=np.uint8)                     # no pixel is 0: a wrongly read pixel shows
    other = np.ascontiguousarray(img[::-1, ::-1])
    mx, my, planted = _planted_maps(W, H)
    want = po.remap_linear(img, mx, my)
    for x, y, axis, v in planted:                                           # what the oracle answers there, from cvRound on x86
        size = W if axis == 0 else H
        if not np.isfinite(v) or abs(v) > 30000 or v >= size or v <= -1:
            assert want[y, x] == 0, (x, y, axis, v)
        elif v in (-0.5, size - 1, size - 0.5):
            assert want[y, x] > 0, (x, y, axis, v)
    assert (want > 0).mean() > 0.9
    cfg = capi.default_config(W, H, orb_nfeatures=200, lsd_nfeatures=0, max_frames=2)
    fe = Frontend(cfg)
    fe.debug_enable(True)
    fe.set_rectify_maps(0, mx, my)
    fe.orb_extract(0, img)
    _assert_level0(fe.debug_fetch(0, capi.DBG_PYRAMID_LEVEL, 0), want, mx, my, planted, "orb_extract")
    # the same maps through the batch path, as frame 1 of two frames
    fe.batch_run_host(np.stack([np.stack([other, other]), np.stack([img, other])]), stages=capi.RUN_ORB)
    _assert_level0(fe.debug_fetch(2, capi.DBG_PYRAMID_LEVEL, 0), want, mx, my, planted, "batch_run_host frame 1")
    assert np.array_equal(fe.debug_fetch(3, capi.DBG_PYRAMID_LEVEL, 0).reshape(H, W), other)     # the eye without maps: a copy
    fe.close()


def _rgbd_numpy(kp, depth, bf):
    """Frame.cc:1309-1331: d = imDepth.at<float>(v, u) with the float coordinates truncated; d > 0 -> mvDepth = d,
    mvuRight = x - bf / d (float32); else both stay -1."""
    d = depth[kp["y"].astype(np.int32), kp["x"].astype(np.int32)]
    with np.errstate(all="ignore"):
        ur = (kp["x"] - np.float32(bf) / d).astype(np.float32)
    ok = d > 0
    return np.where(ok, ur, np.float32(-1)), np.where(ok, d, np.float32(-1))


def test_rgbd_association_special_depths_and_row_stride(gpu):
    capi, Frontend, po = gpu
    from pli_slam_amd import synth
    from pli_slam_amd.capi import check, ptr
    W, H = 128, 96
    cfg = capi.default_config(W, H, orb_nfeatures=200, lsd_nfeatures=0)
    fe = Frontend(cfg)
    L4, _ = synth.make_stereo_pair(3, 4 * W, 4 * H)
    n, kp, _ = fe.orb_extract(0, np.ascontiguousarray(L4[::4, ::4]))
    bf = np.float32(cfg.bf)
    # the depth image is built after the keypoints are known: the cells under them hold the special values in turn
    rng = np.random.default_rng(2)
    depth = rng.uniform(0.3, 8.0, (H, W)).astype(np.float32)
    special = [np.float32(0), np.float32(-0.0), np.float32(-1.5), np.float32(np.nan), np.float32(np.inf),
               np.float32(1.4e-45), np.float32(1e-30), bf, None, None]      # None: the ordinary depth stays
    cells = sorted({(int(y), int(x)) for x, y in zip(kp["x"], kp["y"])})
    assert n > 60 and len(cells) >= 3 * len(special)
    for i, (y, x) in enumerate(cells):
        v = special[i % len(special)]
        if v is not None:
            depth[y, x] = v
    want_ur, want_dp = _rgbd_numpy(kp, depth, bf)
    assert (want_dp == -1).sum() >= 12 and np.isinf(want_dp).any() and (want_dp == bf).any() and np.isneginf(want_ur).any()
    our, odp = po.stereo_from_depth(kp, depth, cfg.bf)                     # the oracle agrees with the five lines too
    assert our.tobytes() == want_ur.tobytes() and odp.tobytes() == want_dp.tobytes()

    ur, dp = fe.stereo_from_depth(depth)
    assert ur[:n].tobytes() == want_ur.tobytes() and dp[:n].tobytes() == want_dp.tobytes()
    assert len(ur) == fe.kp_cap > n and not ur[n:].any() and not dp[n:].any()   # rows beyond the keypoint count: as passed in
    # a row stride larger than the width (the 2-D copy of the C entry point); the pad holds another value
    stride = W + 24
    padded = np.full((H, stride), np.float32(3.25), np.float32)
    padded[:, :W] = depth
    ur2, dp2 = fe.stereo_from_depth(padded, stride=stride)
    assert ur2[:n].tobytes() == want_ur.tobytes() and dp2[:n].tobytes() == want_dp.tobytes()
    # ... and the C entry point writes only the keypoints' rows
    ur3, dp3 = np.full(fe.kp_cap, np.float32(123), np.float32), np.full(fe.kp_cap, np.float32(456), np.float32)
    check(fe.L.pli_stereo_from_depth(fe.h, ptr(padded), C.c_int64(stride), ptr(ur3), ptr(dp3), fe.kp_cap))
    assert ur3[:n].tobytes() == want_ur.tobytes() and dp3[:n].tobytes() == want_dp.tobytes()
    assert (ur3[n:] == 123).all() and (dp3[n:] == 456).all()
    fe.close()
