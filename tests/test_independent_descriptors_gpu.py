"""The independent descriptor checks of test_independent_descriptors.py, run on the KERNELS' own outputs: the keypoint and
descriptor tables, the pyramid and blurred levels (DBG_PYRAMID_LEVEL, DBG_BLUR_LEVEL), the selected keypoints of every level
(DBG_LEVEL_KEYPOINTS), the keylines, the Sobel planes (DBG_LBD_DXDY) and the float LBD vectors (DBG_LBD_FLOAT), all from the
batch entry point with the planes fetched by image index (frame * 2 + eye).

  * ORB: the table angle equals fastAtan2 of the independently summed disk moments and lies within 0.3 degrees of atan2; the
    float32 steered BRIEF (helper trig mode = the context's PARITY_TRIG_F32_ORB) equals the descriptor bit for bit; a float64
    bit that disagrees sits within 1e-4 px of a rounding tie.
  * LBD: DBG_LBD_FLOAT lies within helpers_descriptors.lbd_error_bound of the float64 LBD, and every bit whose float64 margin
    exceeds 4 bounds equals the kernel's bit.

A debug context runs a different LSD schedule, so a product context (dev=False, no debug) must give byte-identical tables
for the same images: the checked tables are the ones the product computes."""
import numpy as np
import pytest

import helpers_descriptors as hd
from pli_slam_amd import capi, realdata, synth

pytestmark = pytest.mark.gpu

TRIG = capi.PARITY_TRIG_F32_ORB | capi.PARITY_TRIG_F32_LBD


@pytest.fixture(scope="module")
def gpu(oracle):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from pli_slam_amd.frontend import Frontend
    return Frontend, oracle


def long_line_frame(seed, W, H):
    """A synthetic frame with a bright bar across the whole width on a clean band (two edges of W - 20 samples) and a
    diagonal above it."""
    L, R = synth.make_stereo_pair(seed, W, H)
    y0 = H // 3
    for img, d in ((L, 0), (R, 12)):
        img[y0 - 60:y0 + 66, :] = 60
        img[y0:y0 + 6, 10:W - 10] = 250
        for k in range(0, 600):
            img[20 + k, 20 + k - d:24 + k - d] = 15
    return L, R


def crop64(y, x):
    """The smallest frame the configuration accepts, 64 x 64, cut from a photograph."""
    L = np.ascontiguousarray(realdata.photos()["camera"][y:y + 64, x:x + 64])
    return L, realdata.shifted_right(L, disparity=3)


def cases():
    c = {}
    c["synth752_x2"] = (lambda: [synth.make_stereo_pair(s, 752, 480) for s in (0, 1)], {}, None)
    c["real752_x3"] = (lambda: realdata.frames_752x480(3, seed=5), {}, None)
    c["odd641x479_trig_set"] = (lambda: [synth.make_stereo_pair(2, 641, 479)], {}, TRIG)
    c["small376x240_trig_clear"] = (lambda: [synth.make_stereo_pair(3, 376, 240)], dict(orb_nfeatures=500, lsd_nfeatures=60), 0)
    c["min64x64"] = (lambda: [crop64(y, x) for y, x in ((180, 200), (250, 150))], dict(orb_nfeatures=100, lsd_nfeatures=20), None)
    c["pyramid1.5x5"] = (lambda: [synth.make_stereo_pair(6, 752, 480)], dict(orb_scale_factor=1.5, orb_nlevels=5), TRIG)
    c["constructed"] = (lambda: [(hd.constructed_image(752, 480, seed=s), hd.constructed_image(752, 480, seed=s + 1))
                                 for s in (3, 7)], {}, 0)
    c["uhd3840x2160"] = (lambda: [long_line_frame(8, 3840, 2160)], dict(orb_nfeatures=4000, lsd_nfeatures=500), None)
    return c


CASES = cases()


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_descriptors_against_independent_restatement(gpu, name):
    Frontend, po = gpu
    make, over, flags = CASES[name]
    frames = make()
    images = np.stack([np.stack([L, R]) for L, R in frames])
    nf, _, H, W = images.shape
    kw = dict(orb_nfeatures=1200, lsd_nfeatures=100)
    kw.update(over)
    cfg = capi.default_config(W, H, max_frames=nf, **kw)
    if flags is not None:
        cfg.parity_flags = (cfg.parity_flags & ~TRIG) | flags
    orb_trig = "cosf" if cfg.parity_flags & capi.PARITY_TRIG_F32_ORB else "cr"
    lbd_trig = "cosf" if cfg.parity_flags & capi.PARITY_TRIG_F32_LBD else "cr"

    fe = Frontend(cfg)
    fe.debug_enable(True)
    recs = fe.batch_run_host(images)
    prod = Frontend(cfg, dev=False)
    precs = prod.batch_run_host(images)
    for f in range(nf):
        for k in ("kpL", "kpR", "descL", "descR", "klL", "klR", "ldescL", "ldescR"):
            assert recs[f][k].tobytes() == precs[f][k].tobytes(), "%s frame %d: %s differs between debug and product" % (name, f, k)
    prod.close()

    dims = hd.level_dims(W, H, cfg.orb_scale_factor, cfg.orb_nlevels)
    tot = dict(kp=0, disagree=0, near_ties=0, flat=0, lines=0, undecided=0, longest=0)
    worst = 0.0
    fails = []
    for f in range(nf):
        for eye, e in ((0, "L"), (1, "R")):
            idx = 2 * f + eye
            kp, desc = recs[f]["kp" + e], recs[f]["desc" + e]
            assert not recs[f]["truncated"][2 + eye]
            base = 0
            for l in range(cfg.orb_nlevels):
                pts = fe.debug_points(idx, capi.DBG_LEVEL_KEYPOINTS, l)
                m = len(pts)
                if not m:
                    continue
                w, h = dims[l]
                lev = fe.debug_fetch(idx, capi.DBG_PYRAMID_LEVEL, l)
                blur = fe.debug_fetch(idx, capi.DBG_BLUR_LEVEL, l)
                assert lev.size == blur.size == w * h, (name, l, lev.size, w, h)
                k = kp[base:base + m]
                assert (k["octave"] == l).all()
                r = hd.check_orb_level(lev.reshape(h, w), blur.reshape(h, w), pts[:, 0] + 16, pts[:, 1] + 16, k["angle"],
                                       desc[base:base + m], orb_trig, po.fast_atan2)
                fails += ["%s frame %d eye %d level %d: %s" % (name, f, eye, l, s) for s in r["fail"]]
                for key in ("disagree", "near_ties", "flat"):
                    tot[key] += r[key]
                tot["kp"] += m
                base += m
            assert base == len(kp), (name, f, eye, base, len(kp))
            kl, ld = recs[f]["kl" + e], recs[f]["ldesc" + e]
            n = len(kl)
            dxy = fe.debug_fetch(idx, capi.DBG_LBD_DXDY).view(np.int16)
            assert dxy.size == 2 * W * H
            lf = fe.debug_fetch(idx, capi.DBG_LBD_FLOAT).view(np.float32).reshape(-1, 72)[:n]
            r = hd.check_lbd(dxy[:W * H].reshape(H, W), dxy[W * H:].reshape(H, W), kl, lf, ld, lbd_trig)
            fails += ["%s frame %d eye %d: %s" % (name, f, eye, s) for s in r["fail"]]
            tot["lines"] += n
            tot["undecided"] += r["undecided"]
            tot["longest"] = max(tot["longest"], int(kl["numOfPixels"].max(initial=0)))
            worst = max(worst, r["worst"])
    fe.close()
    print("%s: %d keypoints (%d flat), %d ORB bits within %.0e px of a tie, %d float64 bits differ; %d lines (longest %d px), "
          "LBD worst error %.3f of the bound, %d undecided bits" % (
              name, tot["kp"], tot["flat"], tot["near_ties"], hd.TIE_MARGIN, tot["disagree"], tot["lines"], tot["longest"],
              worst, tot["undecided"]))
    assert not fails, fails[:5]
    assert tot["kp"] > 0 and tot["lines"] > 0
    if name == "uhd3840x2160":
        assert tot["longest"] >= 3500
    if name == "constructed":
        assert tot["flat"] > 0
