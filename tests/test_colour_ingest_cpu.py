"""The colour and depth conversions of the GrabImage head, without a GPU: known answers of the numpy statement the GPU tests compare
the device with (tests/helpers_ingest.py), and the two new entry points in both builds of the library and in the ctypes binding."""
import ctypes as C

import numpy as np
import pytest

import helpers_ingest as hi


def _px(fmt, r, g, b, a=255):
    p = {hi.RGB8: [r, g, b], hi.BGR8: [b, g, r], hi.RGBA8: [r, g, b, a], hi.BGRA8: [b, g, r, a]}[fmt]
    return np.array([[p]], np.uint8)


@pytest.mark.parametrize("fmt", sorted(hi.FORMATS.values()))
def test_pure_colours_and_grays(fmt):
    # (255 * c + 8192) >> 14 for the three coefficients; the coefficients sum to 2^14, so a gray pixel keeps its value
    assert hi.R2Y + hi.G2Y + hi.B2Y == 1 << 14
    assert [int(hi.gray_of(_px(fmt, *c), fmt)[0, 0]) for c in ((255, 0, 0), (0, 255, 0), (0, 0, 255))] == [76, 150, 29]
    v = np.arange(256, dtype=np.uint8)
    img = np.repeat(v[None, :, None], hi.CHANNELS[fmt], axis=2)
    assert np.array_equal(hi.gray_of(img, fmt)[0], v)


def test_channel_order_and_alpha():
    rng = np.random.default_rng(5)
    rgb = rng.integers(0, 256, (9, 13, 3), dtype=np.uint8)
    want = hi.gray_of(rgb, hi.RGB8)
    assert want.dtype.kind == "i" and want.min() >= 0 and want.max() <= 255
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    assert np.array_equal(want, (r * 4899 + g * 9617 + b * 1868 + 8192) >> 14)
    bgr = np.ascontiguousarray(rgb[..., ::-1])
    assert np.array_equal(hi.gray_of(bgr, hi.BGR8), want)
    assert not np.array_equal(hi.gray_of(rgb, hi.BGR8), want)               # the order matters on this image
    for alpha in (0, 255, None):
        a = rng.integers(0, 256, (9, 13, 1), dtype=np.uint8) if alpha is None else np.full((9, 13, 1), alpha, np.uint8)
        assert np.array_equal(hi.gray_of(np.concatenate([rgb, a], axis=2), hi.RGBA8), want)
        assert np.array_equal(hi.gray_of(np.concatenate([bgr, a], axis=2), hi.BGRA8), want)
    with pytest.raises(ValueError):
        hi.gray_of(rgb, hi.RGBA8)
    with pytest.raises(ValueError):
        hi.gray_of(rgb[..., 0], hi.RGB8)


@pytest.mark.parametrize("fmt", sorted(hi.FORMATS.values()))
def test_near_tie_block_sits_on_both_sides_of_the_rounding(fmt):
    blk = hi.near_tie_block(1024, fmt, seed=fmt)
    s = hi.weighted_sum(blk[None], fmt)[0]
    d = s % 16384
    below, above = d >= 16384 - 1868, d <= 1868
    assert (below | above).all() and below.sum() >= 400 and above.sum() >= 400
    # a conversion that truncates instead (no + 8192) or rounds in float differs on such pixels
    assert ((s - 8192) >> 14 != s >> 14).mean() > 0.4


def test_depth_of():
    raw = np.array([[0, 1, 4999, 5000, 65535]], np.uint16)
    s = np.float32(1) / np.float32(5000)
    d = hi.depth_of(raw, hi.DEPTH_U16, s)
    assert d.dtype == np.float32 and d[0, 0] == 0 and d[0, 3] == np.float32(5000) * s and d[0, 4] == np.float32(65535) * s
    assert hi.depth_of(raw, hi.DEPTH_U16, 1).tobytes() == raw.astype(np.float32).tobytes()
    f = np.array([[0.0, -0.0, np.nan, np.inf, 1e-30, 2.5]], np.float32)
    assert hi.depth_of(f, hi.DEPTH_F32, 1).tobytes() == f.tobytes()
    assert hi.depth_of(f, hi.DEPTH_F32, 0.5)[0, 5] == np.float32(1.25)


def test_both_builds_export_the_setters_and_the_binding_declares_them():
    from pli_slam_amd import capi
    for name in ("pli_set_image_format", "pli_set_depth_format"):
        assert name in capi._PROTOS and name in capi.exported_symbols(), name
        for dev in (False, True):
            fn = getattr(capi.lib(dev=dev), name)
            assert fn.restype is C.c_int32, (name, dev)
    assert capi._PROTOS["pli_set_image_format"][1] == [C.c_void_p, C.c_int32]
    assert capi._PROTOS["pli_set_depth_format"][1] == [C.c_void_p, C.c_int32, C.c_float]
    assert (capi.IMAGE_GRAY8, capi.IMAGE_RGB8, capi.IMAGE_BGR8, capi.IMAGE_RGBA8, capi.IMAGE_BGRA8) == (0, 1, 2, 3, 4)
    assert (capi.DEPTH_F32, capi.DEPTH_U16) == (0, 1)
    assert capi.IMAGE_CHANNELS == hi.CHANNELS
    # a null context is refused without touching a device
    assert capi.lib().pli_set_image_format(None, capi.IMAGE_RGB8) == -1
    assert capi.lib().pli_set_depth_format(None, capi.DEPTH_U16, 1.0) == -1
