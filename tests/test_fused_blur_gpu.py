"""The blurs that live inside their consumers: k_describe blurs the window of its keypoint in LDS (no blurred pyramid plane on the
product path), k_sobel blurs its tile of level 0 (no blurred level-0 plane).  Every output must equal the oracle's, on images small
enough that the windows and tiles cross borders, are narrower than a tile, or are not multiples of the vector widths.

ORB images are uniform noise: FAST fires everywhere, so the octree keeps keypoints at the minimum border distance (19 pixels: the
window of a tap reaches 18 + 3 pixels, two beyond the level) on all four sides of some level — asserted from the oracle's keypoints.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

gpu_test = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from pli_slam_amd import capi, synth
    from pli_slam_amd.frontend import Frontend
    from oracle import pyoracle as po

    class G:
        pass
    g = G()
    g.capi, g.synth, g.Frontend, g.po = capi, synth, Frontend, po
    return g


def ocfg(g, cfg):
    return g.po.Config.from_buffer_copy(bytes(cfg))


def noise(seed, W, H):
    return np.random.RandomState(seed).randint(0, 256, (H, W)).astype(np.uint8)


def blocks(seed, W, H):
    """Rectangles of constant grey under a little noise: straight edges for the line detector on images too small for synth's scenes."""
    rs = np.random.RandomState(seed)
    img = np.full((H, W), 128, np.int32)
    for _ in range(6):
        x0, y0 = rs.randint(0, W - 16), rs.randint(0, H - 16)
        img[y0:y0 + rs.randint(16, H), x0:x0 + rs.randint(16, W)] = rs.randint(0, 256)
    return np.clip(img + rs.randint(-3, 4, (H, W)), 0, 255).astype(np.uint8)


def border_sides(fr, eye, nlevels):
    """Per level: which of the four sides (left, top, right, bottom) hold a selected keypoint at the minimum distance, 19 pixels."""
    out = []
    for l in range(nlevels):
        pts = fr.level_points(eye, l, True)              # (x, y, score) relative to the FAST border (16, 16)
        h, w = fr.pyramid(eye, l).shape
        if len(pts) == 0:
            out.append((False,) * 4)
            continue
        x, y = pts[:, 0] + 16, pts[:, 1] + 16
        out.append((x.min() == 19, y.min() == 19, x.max() == w - 20, y.max() == h - 20))
    return out


# W, H, levels, features, seed: near the smallest images whose last level still has a FAST cell (62 pixels); widths that are no
# multiple of 4 or 64, last levels narrower than one 64-pixel blur tile (64, 63 and 64 pixels wide)
ORB_CASES = [(77, 75, 2, 120, 0), (91, 90, 3, 150, 1), (229, 225, 8, 400, 4)]


@gpu_test
@pytest.mark.parametrize("W,H,nl,nf,seed", ORB_CASES)
def test_orb_small_images(gpu, W, H, nl, nf, seed):
    g = gpu
    capi = g.capi
    cfg = capi.default_config(W, H, orb_nlevels=nl, orb_nfeatures=nf, lsd_nfeatures=20, max_frames=1)
    plain, dbg = g.Frontend(cfg), g.Frontend(cfg)
    dbg.debug_enable(True)
    fr = g.po.Frame(ocfg(g, cfg))
    for eye in (0, 1):
        img = noise(seed + 100 * eye, W, H)
        on, okp, odesc = fr.orb_extract(eye, img)
        assert on > nf // 2 and fr.pyramid(eye, nl - 1).shape[1] <= 64
        if eye == 0:
            sides = border_sides(fr, eye, nl)
            assert any(all(s) for s in sides), sides     # the reflected part of the window is exercised on every side
        n, kp, desc = plain.orb_extract(eye, img)
        assert n == on and kp.tobytes() == okp.tobytes(), "keypoints / angles"
        assert np.array_equal(desc, odesc), "descriptors"
        n2, kp2, desc2 = dbg.orb_extract(eye, img)
        assert n2 == n and kp2.tobytes() == kp.tobytes() and np.array_equal(desc2, desc), "debug context differs"
        for l in range(nl):
            assert np.array_equal(dbg.debug_fetch(eye, capi.DBG_BLUR_LEVEL, l), fr.pyramid(eye, l, True).ravel()), ("blur", l)


@gpu_test
def test_blur_level_needs_debug(gpu):
    g = gpu
    fe = g.Frontend(g.capi.default_config(77, 75, orb_nlevels=2, orb_nfeatures=120, lsd_nfeatures=20, max_frames=1))
    fe.orb_extract(0, noise(0, 77, 75))
    with pytest.raises(g.capi.PliError):
        fe.debug_fetch(0, g.capi.DBG_BLUR_LEVEL, 0)      # the plane is allocated by debug_enable(True), not with the context


@gpu_test
@pytest.mark.parametrize("f32", [True, False])
def test_orb_trig_and_batch(gpu, f32):
    """Both trig forms of the steering; a batch of 3 frames against three single calls (and the oracle)."""
    g = gpu
    capi = g.capi
    W, H, nl, nf = 91, 90, 3, 150
    flags = capi.PARITY_LSD_F64 | (capi.PARITY_TRIG_F32_ORB if f32 else 0)
    cfg = capi.default_config(W, H, orb_nlevels=nl, orb_nfeatures=nf, lsd_nfeatures=20, max_frames=3, parity_flags=flags)
    fe = g.Frontend(cfg)
    frames = np.stack([np.stack([noise(10 + 2 * f, W, H), noise(11 + 2 * f, W, H)]) for f in range(3)])
    recs = fe.batch_run_host(frames, stages=capi.RUN_ORB)
    for f in range(3):
        fr = g.po.Frame(ocfg(g, cfg))
        for eye, k in ((0, "L"), (1, "R")):
            on, okp, odesc = fr.orb_extract(eye, frames[f, eye])
            assert len(recs[f]["kp" + k]) == on and recs[f]["kp" + k].tobytes() == okp.tobytes(), (f, eye)
            assert np.array_equal(recs[f]["desc" + k], odesc), (f, eye)
            n, kp, desc = fe.orb_extract(eye, frames[f, eye])
            assert n == on and kp.tobytes() == okp.tobytes() and np.array_equal(desc, odesc), ("single call", f, eye)


# W not a multiple of 4; W below one 64-pixel tile is not a valid image (64 is the minimum), so the narrowest: one tile and 2 pixels
# of the next (the second tile is narrower than a dword group), and exactly one tile; H below one tile does not exist either (64):
# H = 2 tiles + 1 and H = 2 tiles; W = 1 tile + 1.
LBD_CASES = [(203, 97, 3), (66, 65, 4), (64, 64, 5), (65, 80, 6)]


@gpu_test
@pytest.mark.parametrize("W,H,seed", LBD_CASES)
def test_lbd_small_images(gpu, W, H, seed):
    g = gpu
    capi = g.capi
    cfg = capi.default_config(W, H, orb_nlevels=1, orb_nfeatures=50, lsd_nfeatures=30, max_frames=1)
    fe = g.Frontend(cfg)
    fe.debug_enable(True)
    fr = g.po.Frame(ocfg(g, cfg))
    nlines = 0
    for eye, img in ((0, blocks(seed, W, H)), (1, noise(seed, W, H))):
        n, kl, ld = fe.line_extract(eye, img)
        on, okl, old = fr.line_extract(eye, img)
        raw = fe.debug_fetch(eye, capi.DBG_LBD_DXDY).view(np.int16)
        dx, dy = fr.lbd_dxdy(eye, (H, W))
        assert np.array_equal(raw[:W * H], dx.ravel()) and np.array_equal(raw[W * H:], dy.ravel()), "dx / dy"
        assert n == on and kl.tobytes() == okl.tobytes() and np.array_equal(ld, old), "keylines / LBD descriptors"
        nlines += on
    assert nlines > 0


@gpu_test
def test_lbd_two_frame_batch(gpu):
    g = gpu
    capi = g.capi
    W, H = 203, 97
    cfg = capi.default_config(W, H, orb_nlevels=1, orb_nfeatures=50, lsd_nfeatures=30, max_frames=2)
    fe = g.Frontend(cfg)
    pairs = [g.synth.make_stereo_pair(s, W, H) for s in (7, 8)]
    recs = fe.batch_run_host(np.stack([np.stack(p) for p in pairs]))
    nlines = 0
    for f in range(2):
        fr = g.po.Frame(ocfg(g, cfg))
        for eye, k in ((0, "L"), (1, "R")):
            on, okl, old = fr.line_extract(eye, pairs[f][eye])
            assert len(recs[f]["kl" + k]) == on and recs[f]["kl" + k].tobytes() == okl.tobytes(), (f, eye)
            assert np.array_equal(recs[f]["ldesc" + k], old), (f, eye)
            nlines += on
    assert nlines > 0


def test_window_covers_every_rotated_tap():
    """Host side: the reach the library sized k_describe's window for is not smaller than the largest rounded coordinate of a
    rotated tap, over the 360 whole-degree keypoint angles and both trig forms, in the kernel's float arithmetic."""
    from pli_slam_amd import capi
    from oracle import pyoracle as po
    txt = open(os.path.join(ROOT, "include", "pli_orb_pattern.inc")).read()
    txt = re.sub(r"//[^\n]*", "", txt)
    pat = np.array([int(v) for v in re.findall(r"-?\d+", txt)], np.float32).reshape(-1, 2)
    assert pat.shape == (512, 2)
    dev = capi.lib(dev=True)
    dev.pli_dev_orb_window_reach.restype = C.c_int32
    reach = dev.pli_dev_orb_window_reach()
    worst = 0
    f32 = np.float32
    for deg in range(360):
        ang = f32(deg) * f32(np.pi / 180.0)
        for a, b in ((f32(po.glibc_cosf(float(ang))), f32(po.glibc_sinf(float(ang)))),
                     (f32(np.cos(np.float64(ang))), f32(np.sin(np.float64(ang))))):
            x, y = pat[:, 0], pat[:, 1]
            r = np.rint((x * b).astype(f32) + (y * a).astype(f32))       # ties to even, like cvRound
            c = np.rint((x * a).astype(f32) - (y * b).astype(f32))
            worst = max(worst, int(np.abs(r).max()), int(np.abs(c).max()))
    assert worst == 18                  # the published pattern: (-13, -13) at 45 degrees
    assert reach >= worst
    assert reach <= worst + 1           # ... and not so generous that the window wastes LDS
