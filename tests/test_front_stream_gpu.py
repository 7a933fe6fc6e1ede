"""The streaming form of the LSD front pass (csrc/lsd_f64.hip: k_lsd_front64s) writes what the tiled form (k_lsd_front64) and the
three separate kernels (k_lsd_blur64 -> k_lsd_resize64 -> k_lsd_grad64) write.  (Agreement only: the three forms call the same rule
code, so a wrong rule is wrong in all of them and the counts stay 0.  tests/test_gpu_parity.py compares the three kernels' scaled and
angle planes with the oracle on a debug context, at whole-frame sizes; what pins every form's planes to the oracle at the sizes below
is tests/test_lsd_front_planes_gpu.py.)
pli_selftest_front_stream runs the three on a batch of images and counts, on the device, the 4-byte words in which they differ — the
hot records, the {cos, sin} plane, the norm plane with its pad columns, the largest norm per image; or, with records=True, the 16-byte
records and the owner plane in place of the first two.  Every count must be 0.

Sizes (source pixels, scale 1.2 unless stated): widths 53 / 54 / 107 / 75 give scaled widths 64 (one strip, no 65th column), 65 (a
second strip of one pixel), 128 (two full strips, pitch = width) and 90 (pad columns 90 .. 95); the heights follow the chunk height
h the library reports (scaled rows per wave): scaled heights below h, h, h + 1 and at least 3h + 5 (a first, an inner and a last
chunk, the last one short)."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

WIDTHS = {53: 64, 54: 65, 107: 128, 75: 90}         # source width -> scaled width at 1.2
ZERO = (0, 0, 0, 0)


def scaled(n, scale=1.2):
    return int(round(n * scale))                      # (cvRound: nearest, ties to even — as Python's round)


def source_for(target, scale=1.2, at_least=False):
    """The source length whose scaled length is `target` (the smallest one that reaches it, with at_least)."""
    for n in range(1, 4096):
        if scaled(n, scale) == target or (at_least and scaled(n, scale) >= target):
            return n
    raise AssertionError("no source length scales to %d" % target)


@pytest.fixture(scope="module")
def fe():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from pli_slam_amd import capi
    from pli_slam_amd.frontend import Frontend
    return Frontend(capi.default_config(128, 128))


@pytest.fixture(scope="module")
def chunk(fe):
    return fe.selftest_front_stream(np.zeros((1, 16, 16), np.uint8))["chunk"]


@pytest.fixture(scope="module")
def photo():
    return np.load(os.path.join(ROOT, "tests", "golden", "real", "photos.npz"))["camera"]


def noise(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def checker(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return (((yy + xx) & 1) * 255).astype(np.uint8)


def batches(photo, h, w):
    """Two batches of three images of different content: a wrong image stride shows as a difference in the second or third."""
    crop = np.ascontiguousarray(photo[100:100 + h, 200:200 + w])
    assert crop.shape == (h, w)
    yield "noise/constant/checker", np.stack([noise(7 * h + w, h, w), np.full((h, w), 131, np.uint8), checker(h, w)])
    yield "photo/checker/noise", np.stack([crop, checker(h, w), noise(11 * h + w + 1, h, w)])


def heights(chunk, scale=1.2):
    below = source_for(max(chunk // 2, 9), scale, at_least=True)
    assert scaled(below, scale) < chunk
    return [below, source_for(chunk, scale), source_for(chunk + 1, scale), source_for(3 * chunk + 5, scale, at_least=True)]


def check(fe, imgs, what, scale=1.2, applied=True):
    for pack_w in (False, True):
        r = fe.selftest_front_stream(imgs, scale=scale, pack_w=pack_w)
        print(what, "pack_w", pack_w, r)
        assert r["applied"] == applied, (what, r)
        assert r["vs_tiled"] == ZERO, (what, pack_w, r)
        assert r["vs_unfused"] == ZERO, (what, pack_w, r)


@pytest.mark.parametrize("w", sorted(WIDTHS))
def test_streaming_front_equals_tiled_and_unfused(fe, chunk, photo, w):
    assert scaled(w) == WIDTHS[w]
    hs = heights(chunk)
    assert [scaled(h) for h in hs][1:3] == [chunk, chunk + 1] and scaled(hs[3]) >= 3 * chunk + 5
    for h in hs:
        for name, imgs in batches(photo, h, w):
            check(fe, imgs, "%dx%d %s" % (w, h, name))


@pytest.mark.parametrize("scale", [1.5, 2.0])
def test_streaming_front_other_scales(fe, chunk, photo, scale):
    w, h = 75, source_for(chunk + 1, scale, at_least=True)
    for name, imgs in batches(photo, h, w):
        check(fe, imgs, "%dx%d x%.1f %s" % (w, h, scale, name), scale=scale)


@pytest.mark.parametrize("w", [54, 75])
def test_forms_agree_on_records_and_owner_plane(fe, chunk, photo, w):
    """The schedules off the hot records (16-byte-record schedules, the sequential schedule, lsd_mode 1) take the 16-byte records —
    with the owner word in rec.w where there is no hot record — and the owner plane's start value from whichever form the context
    chose: the forms must agree on those too.  Scaled widths 65 (a second strip of one pixel) and 90 (pad columns 90 .. 95), the
    scaled height chunk + 1 (a chunk boundary inside the image)."""
    h = source_for(chunk + 1)
    assert scaled(w) == WIDTHS[w] and scaled(h) == chunk + 1
    for name, imgs in batches(photo, h, w):
        for pack_w in (False, True):
            r = fe.selftest_front_stream(imgs, scale=1.2, pack_w=pack_w, records=True)
            print("%dx%d %s" % (w, h, name), "records, pack_w", pack_w, r)
            assert r["applied"], (name, r)
            assert r["vs_tiled"] == ZERO, (name, pack_w, r)
            assert r["vs_unfused"] == ZERO, (name, pack_w, r)


def test_constant_image_has_no_defined_pixel(fe):
    """(what the counts of a constant image rest on: every pixel undefined and the largest norm 0 in all three forms — the selftest
    compares words, so the three agree on exactly that)"""
    check(fe, np.full((3, 40, 53), 17, np.uint8), "constant")


def test_small_image_keeps_the_tiled_form(fe):
    """One reflection at the border needs more than 6 source rows and columns: below that the host keeps the tiled form, which must agree
    with the three kernels."""
    imgs = np.stack([noise(1, 6, 6), checker(6, 6), np.full((6, 6), 200, np.uint8)])
    check(fe, imgs, "6x6", applied=False)
