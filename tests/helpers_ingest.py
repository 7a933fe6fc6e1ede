"""What the GrabImage conversions are, in numpy, for the colour-ingest tests (tests/test_colour_ingest_cpu.py, _gpu.py): no library call.

  gray_of(img, fmt)               OpenCV 3.3.1's C++ path RGB2Gray<uchar> (imgproc/src/color.cpp): 14-bit coefficients R2Y = 4899,
                                  G2Y = 9617, B2Y = 1868, gray = (R*4899 + G*9617 + B*1868 + 8192) >> 14 in integers, alpha not read;
                                  (H, W, 3 | 4) u8 -> (H, W) int64 (every value is in 0 .. 255)
  depth_of(raw, type, scale)      imDepth.convertTo(imDepth, CV_32F, scale): cvtScale with shift 0, one float product per element
                                  ((float)raw * scale, every uint16 is exact in float) -> float32; a float map times 1 is itself
  colour_remap(img, mapx, mapy)   the driver's cv::remap on a colour image (stereo_euroc.cc:166-167): oracle.remap_linear on each
                                  channel, each rounded to 8 bits on its own
  near_tie_block(n, fmt)          n pixels whose weighted sum R*4899 + G*9617 + B*1868 + 8192 lies within 1868 of a multiple of 16384,
                                  half of them just below and half just at or above it: where a rounding that differs shows
"""
import numpy as np

GRAY8, RGB8, BGR8, RGBA8, BGRA8 = range(5)                 # pli_image_format
FORMATS = {"rgb": RGB8, "bgr": BGR8, "rgba": RGBA8, "bgra": BGRA8}
CHANNELS = {GRAY8: 1, RGB8: 3, BGR8: 3, RGBA8: 4, BGRA8: 4}
DEPTH_F32, DEPTH_U16 = 0, 1                                # pli_depth_type
R2Y, G2Y, B2Y, SHIFT = 4899, 9617, 1868, 14


def _rgb_planes(img, fmt):
    img = np.asarray(img)
    if fmt not in (RGB8, BGR8, RGBA8, BGRA8) or img.ndim != 3 or img.shape[2] != CHANNELS[fmt] or img.dtype != np.uint8:
        raise ValueError("(H, W, %s) u8 image expected" % CHANNELS.get(fmt, "?"))
    p = img.astype(np.int64)
    r, b = (p[..., 0], p[..., 2]) if fmt in (RGB8, RGBA8) else (p[..., 2], p[..., 0])
    return r, p[..., 1], b


def weighted_sum(img, fmt):
    r, g, b = _rgb_planes(img, fmt)
    return r * R2Y + g * G2Y + b * B2Y + (1 << (SHIFT - 1))


def gray_of(img, fmt):
    return weighted_sum(img, fmt) >> SHIFT


def depth_of(raw, type, scale):
    raw = np.asarray(raw)
    scale = np.float32(scale)
    if type == DEPTH_U16:
        assert raw.dtype == np.uint16
        return (raw.astype(np.float32) * scale).astype(np.float32)
    assert type == DEPTH_F32 and raw.dtype == np.float32
    if scale == np.float32(1):
        return raw.copy()
    with np.errstate(all="ignore"):
        return (raw * scale).astype(np.float32)


def colour_remap(img, mapx, mapy):
    from oracle import pyoracle as po
    img = np.asarray(img)
    out = img.copy()
    for c in range(3):                  # (an alpha channel stays: nothing reads it)
        out[..., c] = po.remap_linear(np.ascontiguousarray(img[..., c]), mapx, mapy)
    return out


def near_tie_block(n, fmt, seed=0):
    """(n, channels) u8 pixels: for each, G and B are drawn, then R is the value that brings the weighted sum closest to a multiple of
    16384 from below (even rows) or from above (odd rows); kept when the distance is within 1868, drawn again otherwise."""
    rng = np.random.default_rng(seed)
    ch = CHANNELS[fmt]
    out = np.zeros((n, ch), np.uint8)
    k, below, above = 0, 0, 0
    while k < n:
        g, b, a = (int(v) for v in rng.integers(0, 256, 3))
        rest = g * G2Y + b * B2Y + (1 << (SHIFT - 1))
        want_below = k % 2 == 0
        # the multiple of 16384 next above `rest`, reached by R from below (largest R staying under it) or from above (smallest R reaching it)
        for m in range(rest // (1 << SHIFT) + 1, rest // (1 << SHIFT) + 80):
            need = m * (1 << SHIFT) - rest
            r = (need - 1) // R2Y if want_below else -(-need // R2Y)
            if not 0 <= r <= 255:
                continue
            s = rest + r * R2Y
            dist = m * (1 << SHIFT) - s if want_below else s - m * (1 << SHIFT)
            if (0 < dist <= B2Y) if want_below else (0 <= dist <= B2Y):
                px = [r, g, b] if fmt in (RGB8, RGBA8) else [b, g, r]
                out[k, :3] = px
                if ch == 4:
                    out[k, 3] = a
                below += want_below
                above += not want_below
                k += 1
                break
    s = weighted_sum(out[None], fmt)[0]
    d = s % (1 << SHIFT)
    assert below >= n // 2 and above >= n // 2 and (np.minimum(d, (1 << SHIFT) - d) <= B2Y).all()
    return out
