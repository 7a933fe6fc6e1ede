"""Colour images and raw depth maps through the library: pli_set_image_format / pli_set_depth_format (the head of
Tracking::GrabImageStereo / RGBD / Monocular, Tracking.cc:889-914, :964-980, :1014-1027, on the device).

1. Level 0 of the pyramid equals tests/helpers_ingest.py gray_of, byte for byte, for the four formats and three host layouts (tight rows,
   rows padded to a stride that is no multiple of 4, a base pointer one byte into a buffer) — and, with device pointers, for a base
   one byte into a device buffer with such a stride, where k_ingest_colour itself takes its byte path.
2. Whole paths against the path the library had before: frame_extract_single, frame_extract, batch_run_host, the pipelined host
   submit, orb_extract_lapping and line_extract on colour input give the bytes that a second context with the default format gives
   on gray_of(input); back on GRAY8 the first context gives them again on the gray input.
3. With rectification maps on one eye, level 0 is gray_of of the remapped colour image (each channel remapped and rounded on its
   own), the reference's order; the other eye is not remapped.
4. Depth: uint16 maps with scale 1/5000 and 1, float maps with scale 0.5 and 1, a padded stride, against the default context fed
   helpers_ingest.depth_of.
5. Errors, each before anything is launched.

Contexts of 128 x 96 and 131 x 97 (a width that is no multiple of the 4 pixels a thread stores; 131 * 3 bytes per row is no multiple
of 4 either, so three rows in four start off a dword boundary in the staging buffer).  The colour images are photographs, another
one or another shift per channel, plus noise, with a block of pixels whose weighted sum lies next to a rounding step on either side.
"""
import ctypes as C

import numpy as np
import pytest

import helpers_ingest as hi

pytestmark = pytest.mark.gpu

SIZES = [(128, 96), (131, 97)]
RGBD = (0, 0)                              # the lapping area of the RGB-D constructor (Frame.cc:258)
SCALE_TUM = np.float32(1) / np.float32(5000)


def colour_image(W, H, fmt, seed):
    """(H, W, channels) u8: red, green and blue from different photographs / shifts plus noise, alpha random; rows 0 .. 8 hold
    near_tie_block's pixels (at least 1000 of them)."""
    from pli_slam_amd import realdata
    ph = realdata.photos()
    rng = np.random.default_rng(seed)
    y0, x0 = 120 + 7 * seed, 140 + 5 * seed
    planes = [ph["camera"][y0:y0 + H, x0:x0 + W], ph["camera"][y0 + 1:y0 + 1 + H, x0 + 2:x0 + 2 + W], ph["astronaut"][y0:y0 + H, x0:x0 + W]]
    rgb = [np.clip(p.astype(np.int32) + rng.integers(-6, 7, (H, W)), 0, 255).astype(np.uint8) for p in planes]
    ch = hi.CHANNELS[fmt]
    img = np.zeros((H, W, ch), np.uint8)
    order = (0, 1, 2) if fmt in (hi.RGB8, hi.RGBA8) else (2, 1, 0)
    for c, src in zip(order, rgb):
        img[..., c] = src
    if ch == 4:
        img[..., 3] = rng.integers(0, 256, (H, W), dtype=np.uint8)
    rows = -(-1000 // W)
    img[:rows] = hi.near_tie_block(rows * W, fmt, seed=seed).reshape(rows, W, ch)
    return img


def layouts(img):
    """The image in three host layouts: name -> an (H, W, ch) view with the same pixels."""
    H, W, ch = img.shape
    stride = W * ch + 5
    if stride % 4 == 0:
        stride += 1
    padded = np.full((H, stride), 0xA5, np.uint8)
    padded[:, :W * ch] = img.reshape(H, W * ch)
    buf = np.full(H * W * ch + 1, 0x5A, np.uint8)
    buf[1:] = img.ravel()
    out = {"tight": img, "padded": padded[:, :W * ch].reshape(H, W, ch), "offset": buf[1:].reshape(H, W, ch)}
    assert out["padded"].strides == (stride, ch, 1) and stride % 4 != 0 and out["offset"].ctypes.data % 4 != 0
    return out


@pytest.fixture(scope="module", params=SIZES, ids=["%dx%d" % s for s in SIZES])
def ctx(request):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from pli_slam_amd import capi
    from pli_slam_amd.frontend import Frontend
    W, H = request.param
    cfg = capi.default_config(W, H, orb_nfeatures=300, lsd_nfeatures=50, max_frames=2)
    col, ref = Frontend(cfg), Frontend(cfg)
    yield dict(capi=capi, Frontend=Frontend, cfg=cfg, col=col, ref=ref, W=W, H=H)
    col.close()
    ref.close()


def _gray(img, fmt):
    return hi.gray_of(img, fmt).astype(np.uint8)


def _same_records(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        if k == "full":
            for kk in a[k]:
                assert a[k][kk].tobytes() == b[k][kk].tobytes(), (what, "full", kk)
        elif isinstance(a[k], np.ndarray):
            assert a[k].tobytes() == b[k].tobytes(), (what, k)
        else:
            assert a[k] == b[k], (what, k)


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(hi.FORMATS))
def test_level_0_is_the_gray_image_byte_for_byte(ctx, name):
    fmt, col = hi.FORMATS[name], ctx["col"]
    img = colour_image(ctx["W"], ctx["H"], fmt, seed=fmt)
    want = _gray(img, fmt)
    ties = hi.weighted_sum(img, fmt) % 16384
    assert (np.minimum(ties, 16384 - ties) <= 1868).sum() >= 1000
    col.set_image_format(fmt)
    for lay, view in layouts(img).items():
        n, _, _ = col.orb_extract(0, view)
        got = col.pyramid_level(0, 0)
        bad = np.argwhere(got != want)
        assert not len(bad), "%s, %s rows: %d pixels differ, first (y, x, device, numpy): %s" % (
            name, lay, len(bad), [(int(y), int(x), int(got[y, x]), int(want[y, x])) for y, x in bad[:6]])
        assert n > 20, (name, lay, n)
    col.set_image_format(hi.GRAY8)


@pytest.mark.parametrize("name", ["rgb", "bgra"])
def test_device_images_at_an_odd_base_and_a_stride_off_the_dwords(ctx, name):
    """pli_batch_run with device pointers: no staging copy lies between the caller's layout and the kernel, so an odd base and a
    stride that is no multiple of 4 reach k_ingest_colour itself."""
    import torch
    fmt, col, ref, W, H = hi.FORMATS[name], ctx["col"], ctx["ref"], ctx["W"], ctx["H"]
    ch = hi.CHANNELS[fmt]
    imgs = [[colour_image(W, H, fmt, seed=10 * f + e) for e in range(2)] for f in range(2)]
    stride = W * ch + 3 + (1 if (W * ch + 3) % 4 == 0 else 0)
    host = np.full(1 + 2 * 2 * H * stride, 0xC3, np.uint8)
    body = host[1:].reshape(2, 2, H, stride)
    for f in range(2):
        for e in range(2):
            body[f, e, :, :W * ch] = imgs[f][e].reshape(H, W * ch)
    dimg = torch.from_numpy(host).cuda()
    dtab = torch.zeros(col.table_bytes(2), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    base = dimg.data_ptr() + 1
    assert base % 2 == 1 and stride % 4 != 0
    col.set_image_format(fmt)
    col.batch_run_device(2, base, base + H * stride, stride, 2 * H * stride, dtab.data_ptr())
    col.sync()
    tab = dtab.cpu().numpy()
    col.set_image_format(hi.GRAY8)
    want = ref.batch_run_host(np.stack([np.stack([_gray(imgs[f][e], fmt) for e in range(2)]) for f in range(2)]))
    for f in range(2):
        _same_records(col.parse_record(tab, f), want[f], "%s frame %d" % (name, f))
    assert len(want[0]["kpL"]) > 20 and len(want[1]["kpR"]) > 20


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(hi.FORMATS))
def test_whole_paths_equal_the_gray_path_of_a_default_context(ctx, name):
    fmt, col, ref, W, H = hi.FORMATS[name], ctx["col"], ctx["ref"], ctx["W"], ctx["H"]
    left, right = colour_image(W, H, fmt, seed=1), colour_image(W, H, fmt, seed=2)
    gl, gr = _gray(left, fmt), _gray(right, fmt)
    lay = layouts(left)
    col.set_image_format(fmt)
    got = {
        "single": col.frame_extract_single(lay["padded"], RGBD),
        "frame": col.frame_extract(lay["offset"], right),
        "batch": col.batch_run_host(np.stack([np.stack([left, right]), np.stack([right, left])])),
        "lapping": col.orb_extract_lapping(0, left, (0, 1000)),
        "lines": col.line_extract(1, right),
    }
    hl, hr, tables = col.host_buffers(2)
    hl[0], hl[1], hr[0], hr[1] = left.ravel(), right.ravel(), right.ravel(), left.ravel()
    col.host_submit(2, hl, hr, tables[0])
    with pytest.raises(ctx["capi"].PliError) as e:               # refused while the batch has not been waited for
        col.set_image_format(hi.GRAY8)
    assert e.value.status == -1
    col.host_wait_all()
    got["submit"] = [col.parse_record(tables[0], f) for f in range(2)]
    col.set_image_format(hi.GRAY8)

    def gray_path(fe):
        return {
            "single": fe.frame_extract_single(gl, RGBD),
            "frame": fe.frame_extract(gl, gr),
            "batch": fe.batch_run_host(np.stack([np.stack([gl, gr]), np.stack([gr, gl])])),
            "lapping": fe.orb_extract_lapping(0, gl, (0, 1000)),
            "lines": fe.line_extract(1, gr),
        }

    for who, fe in (("the default context", ref), ("the first context back on GRAY8", col)):
        want = gray_path(fe)
        _same_records(got["single"], want["single"], (who, "frame_extract_single"))
        _same_records(got["frame"], want["frame"], (who, "frame_extract"))
        for f in range(2):
            _same_records(got["batch"][f], want["batch"][f], (who, "batch_run_host", f))
            _same_records(got["submit"][f], want["batch"][f], (who, "host_submit", f))
        for k in ("lapping", "lines"):
            assert len(got[k]) == len(want[k])
            for a, b in zip(got[k], want[k]):
                assert (a.tobytes() == b.tobytes()) if isinstance(a, np.ndarray) else a == b, (who, k)
    r = got["frame"]
    assert len(r["kpL"]) > 20 and len(r["kpR"]) > 20 and len(r["klL"]) > 2 and len(got["single"]["kpL"]) > 20


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------
def _maps(W, H):
    """A rotation by 1.5 degrees about the centre, with a few coordinates far outside the image, infinite and NaN."""
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
    a = np.float32(np.deg2rad(1.5))
    c, s = np.float32(np.cos(a)), np.float32(np.sin(a))
    cx, cy = np.float32(W / 2), np.float32(H / 2)
    mx = (c * (xs - cx) - s * (ys - cy) + cx).astype(np.float32)
    my = (s * (xs - cx) + c * (ys - cy) + cy).astype(np.float32)
    for i, v in enumerate((-40000.0, 40000.0, 7e7, -1e9, np.inf, -np.inf, np.nan, -1.0, W + 0.0)):
        mx[20 + 5 * i, (11 * i + 3) % W] = np.float32(v)
        my[22 + 5 * i, (13 * i + W - 4) % W] = np.float32(v)
    return mx, my


@pytest.mark.parametrize("name", ["rgb", "bgra"])
def test_rectification_remaps_the_colour_image_then_converts(ctx, name):
    fmt, W, H = hi.FORMATS[name], ctx["W"], ctx["H"]
    fe = ctx["Frontend"](ctx["cfg"])
    try:
        img = colour_image(W, H, fmt, seed=3)
        mx, my = _maps(W, H)
        want = _gray(hi.colour_remap(img, mx, my), fmt)
        plain = _gray(img, fmt)
        # converting first and remapping the gray image is another function: it must differ somewhere, or the test shows nothing
        from oracle import pyoracle as po
        assert (po.remap_linear(plain, mx, my) != want).any()
        fe.set_image_format(fmt)
        fe.set_rectify_maps(0, mx, my)
        fe.orb_extract(0, img)
        fe.orb_extract(1, img)
        got0, got1 = fe.pyramid_level(0, 0), fe.pyramid_level(1, 0)
        bad = np.argwhere(got0 != want)
        assert not len(bad), "%d pixels differ, first (y, x, device, numpy): %s" % (
            len(bad), [(int(y), int(x), int(got0[y, x]), int(want[y, x])) for y, x in bad[:6]])
        assert np.array_equal(got1, plain)                          # the eye without maps
        assert (want == 0).sum() >= 10 and (want > 0).mean() > 0.8
    finally:
        fe.close()


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------
def _raw_depth(W, H, kp):
    """uint16: a ramp with a band of 0; 65535, 0, 1 and ordinary values in turn under the keypoints; the last row and the last column
    hold values of their own."""
    ys, xs = np.mgrid[0:H, 0:W]
    raw = (3000 + 41 * xs + 173 * ys).astype(np.uint16)
    raw[40:48] = 0
    raw[H - 1, :] = 60000 + np.arange(W)
    raw[:, W - 1] = 50000 + np.arange(H)
    cells = sorted({(int(y), int(x)) for x, y in zip(kp["x"], kp["y"])})
    for i, (y, x) in enumerate(cells):
        v = (65535, 0, 1, None, None)[i % 5]
        if v is not None:
            raw[y, x] = v
    return raw


def test_depth_formats_equal_the_converted_map_on_a_default_context(ctx):
    capi, col, ref, W, H = ctx["capi"], ctx["col"], ctx["ref"], ctx["W"], ctx["H"]
    fmt = hi.RGB8
    img = colour_image(W, H, fmt, seed=4)
    gray = _gray(img, fmt)
    col.set_image_format(fmt)
    try:
        n, kp, _ = col.orb_extract(0, img)
        n2, kp2, _ = ref.orb_extract(0, gray)
        assert n == n2 > 20 and kp.tobytes() == kp2.tobytes()
        raw = _raw_depth(W, H, kp)
        under = raw[kp["y"].astype(np.int32), kp["x"].astype(np.int32)]
        assert (under == 0).any() and (under == 65535).any() and (under == 1).any()
        stride = W + 7
        padded = np.full((H, stride), 4242, np.uint16)
        padded[:, :W] = raw
        flt = hi.depth_of(raw, hi.DEPTH_U16, np.float32(0.37))
        cells = sorted({(int(y), int(x)) for x, y in zip(kp["x"], kp["y"])})
        for i, v in enumerate((np.nan, np.inf, -0.0, -2.5, 1e-30)):
            flt[cells[(5 * i + 3) % len(cells)]] = np.float32(v)
        cases = [("U16 x 1/5000", hi.DEPTH_U16, SCALE_TUM, raw, None), ("U16 x 1", hi.DEPTH_U16, np.float32(1), raw, None),
                 ("U16 x 1/5000, padded rows", hi.DEPTH_U16, SCALE_TUM, padded, stride), ("F32 x 0.5", hi.DEPTH_F32, np.float32(0.5), flt, None),
                 ("F32 x 1", hi.DEPTH_F32, np.float32(1), flt, None)]
        for what, typ, scale, src, st in cases:
            conv = hi.depth_of(src, typ, scale)
            if what == "F32 x 1":
                assert conv.tobytes() == src.tobytes()
            col.set_depth_format(typ, scale)
            col.orb_extract(0, img)
            ref.orb_extract(0, gray)
            ur, dp = col.stereo_from_depth(src, stride=st)
            wur, wdp = ref.stereo_from_depth(conv, stride=st)
            assert ur.tobytes() == wur.tobytes() and dp.tobytes() == wdp.tobytes(), what
            d = conv[kp["y"].astype(np.int32), kp["x"].astype(np.int32)]
            assert (dp[:n][d > 0] == d[d > 0]).all() and (dp[:n][~(d > 0)] == -1).all() and (d > 0).sum() > 10, what
            got = col.frame_extract_single(img, RGBD, src)
            want = ref.frame_extract_single(gray, RGBD, conv)
            _same_records(got, want, what)
            assert (got["depth"] > 0).sum() > 10 and (got["depth"] == -1).any(), what
        with pytest.raises(ValueError):
            col.set_depth_format(hi.DEPTH_U16, SCALE_TUM)
            col.stereo_from_depth(flt)                              # a float map under DEPTH_U16
    finally:
        col.set_depth_format(hi.DEPTH_F32, 1.0)
        col.set_image_format(hi.GRAY8)


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------
def test_errors_come_before_anything_is_launched(ctx):
    capi, W, H = ctx["capi"], ctx["W"], ctx["H"]
    fe = ctx["Frontend"](ctx["cfg"])
    try:
        L = fe.L
        img = colour_image(W, H, hi.RGB8, seed=6)
        rgba = colour_image(W, H, hi.RGBA8, seed=6)
        # a 3-D array under GRAY8, a 2-D one or the wrong channel count under a colour format: refused by the helper
        for f, bad in ((hi.GRAY8, img), (hi.RGB8, img[..., 0]), (hi.RGB8, rgba), (hi.BGRA8, img)):
            fe.set_image_format(f)
            with pytest.raises(ValueError):
                fe.orb_extract(0, bad)
            with pytest.raises(ValueError):
                fe.frame_extract_single(bad, RGBD)
        # unknown enums
        for call in (lambda: fe.set_image_format(5), lambda: fe.set_image_format(-1), lambda: fe.set_depth_format(2, 1.0),
                     lambda: fe.set_depth_format(hi.DEPTH_U16, np.inf)):
            with pytest.raises(capi.PliError) as e:
                call()
            assert e.value.status == -1
        assert fe.image_format == hi.BGRA8 and fe.depth_type == hi.DEPTH_F32        # a refused setting changes nothing
        # stride < w * channels at every entry point that takes images
        fe.set_image_format(hi.RGB8)
        n, mono = C.c_int32(), C.c_int32()
        kp, desc = np.zeros(fe.kp_cap, capi.KEYPOINT_DT), np.zeros((fe.kp_cap, 32), np.uint8)
        kl = np.zeros(fe.kl_cap, capi.KEYLINE_DT)
        rec = np.zeros(fe.table_bytes(2), np.uint8)
        un, ln, cell = np.zeros((fe.kp_cap, 2), np.float32), np.zeros((fe.kl_cap, 4), np.float32), np.zeros(fe.kp_cap, np.int32)
        p, short = capi.ptr(img), 3 * W - 1
        assert L.pli_orb_extract(fe.h, 0, p, W, H, short, capi.ptr(kp), fe.kp_cap, capi.ptr(desc), C.byref(n)) == -1
        assert L.pli_orb_extract(fe.h, 0, p, W, H, W, capi.ptr(kp), fe.kp_cap, capi.ptr(desc), C.byref(n)) == -1     # the gray stride
        assert L.pli_orb_extract_lapping(fe.h, 0, p, W, H, short, 0, 0, capi.ptr(kp), fe.kp_cap, capi.ptr(desc), C.byref(n), C.byref(mono)) == -1
        assert L.pli_line_extract(fe.h, 0, p, W, H, short, capi.ptr(kl), fe.kl_cap, capi.ptr(desc), C.byref(n)) == -1
        assert L.pli_frame_extract(fe.h, p, p, W, H, 3 * W, short, capi.ptr(rec)) == -1
        assert L.pli_frame_extract_single(fe.h, p, W, H, short, 0, 0, None, 0, capi.ptr(rec), capi.ptr(un), capi.ptr(ln), capi.ptr(cell),
                                          C.byref(mono)) == -1
        assert L.pli_batch_run_host(fe.h, 1, p, p, short, 3 * W * H, capi.RUN_ALL, capi.ptr(rec)) == -1
        assert L.pli_batch_submit_host(fe.h, 1, p, p, short, 3 * W * H, capi.RUN_ALL, capi.ptr(rec)) == -1
        assert L.pli_batch_run(fe.h, 1, p, p, short, 3 * W * H, capi.RUN_ALL, capi.ptr(rec)) == -1       # (refused before the pointers are used)
        # nothing ran: no eye has been extracted on this context
        counts = (C.c_int32 * 4)()
        capi.check(L.pli_last_counts(fe.h, counts))
        assert list(counts) == [-1, -1, -1, -1]
        with pytest.raises(capi.PliError) as e:
            fe.pyramid_level(0, 0)
        assert e.value.status == -6
    finally:
        fe.close()
