"""region2rect with its fetches issued a block at a time (pli_slam_amd/csrc/lsd_rect.hpp, PRE): the list entries of a block back to
back, then the weights, then the ordered sums from registers.  Only WHEN a load is issued changed, so every segment stays the
oracle's, byte for byte — in key mode (the product library) and in rank mode (development build, PLI_TX_KEYS=0), on single frames
and on the second, look-free call of a batch context, where the later rounds' k_rx_rect launches and k_tx_tail (which keeps the
chunk-by-chunk form) produce segments too.

The image is made of noise-free bars (helpers_line_ref.bars_image) whose lengths, thicknesses and contrasts were chosen so that the
sequential grower ends with regions of exactly n - 1, n and n + 1 pixels for every n at which the code changes path:
  16, 32, 48, 64   the chunks of a 16-lane group
  96               a group's half block (6 of its 12 chunks) against the whole one
  192              RX_RECT_GROUP_MAX: 16-lane groups hand over to the whole wave
  256, 512         RX_RECT_WAVE_BLOCK chunks of 64: one and two blocks of the whole wave
  384              the whole wave's half block (its second block ends within 128 pixels) against the whole one
The sizes are asserted twice: on a restatement of the oracle's region_grow over the oracle's own angle plane and visiting order
(it must give as many regions of minRegSize pixels as the oracle lists segments), and on PLI_DBG_LSD_SIZES of a debug context,
where every region of at least minRegSize pixels goes to region2rect."""
import math

import numpy as np
import pytest

from helpers_line_ref import bars_image

pytestmark = pytest.mark.gpu

W, H = 376, 240
PATH_CHANGES = (16, 32, 48, 64, 96, 192, 256, 384, 512)
SIZES = tuple(n + d for n in PATH_CHANGES for d in (-1, 0, 1))
TABLES = ("klL", "klR", "ldescL", "ldescR", "disp", "le")
# (x0, x1, y, thickness, hi): rows 24 px apart, x0 and y on the phases (mod 6: the scale is 1.2) at which the sizes come out
BARS = ((9, 153, 12, 2, 200), (182, 290, 12, 3, 200),
        (9, 117, 39, 4, 200), (143, 209, 37, 8, 200), (234, 289, 39, 4, 200),
        (6, 61, 60, 3, 200), (89, 143, 60, 2, 200), (170, 224, 60, 2, 200), (253, 281, 60, 2, 200), (305, 323, 60, 6, 200),
        (9, 37, 87, 2, 200), (61, 76, 84, 3, 200), (104, 119, 84, 5, 200), (143, 155, 84, 5, 200), (182, 192, 84, 6, 200),
        (218, 228, 85, 8, 200), (254, 264, 84, 2, 200), (289, 295, 84, 8, 200),
        (9, 117, 111, 2, 200), (6, 78, 132, 2, 200), (6, 61, 156, 2, 200), (9, 170, 204, 4, 70))


def bars(shift=0):
    img = np.full((H, W), 40, np.uint8)
    for x0, x1, y, t, hi in BARS:
        img = np.maximum(img, bars_image(W, H, x0 + shift, x1 + shift, (y,), t, 40, hi))
    return img


def grower_sizes(po, fr, eye):
    """line_oracle.hpp region_grow restated on the oracle's angle plane and order: (the size of every region, minRegSize)"""
    deg = fr.lsd_angle(eye)
    h, w = deg.shape
    ang = deg.astype(np.float64).ravel() * (math.pi / 180)
    defined = deg.ravel() != -1024.0
    trig = po.lsd_pixel_trig(deg, False).reshape(-1, 2)
    prec = math.pi * 22.5 / 180
    log_nt = 5 * (math.log10(w) + math.log10(h)) / 2 + math.log10(11.0)
    min_reg = int(-log_nt / math.log10(22.5 / 180))
    used = ~defined
    sizes = []
    for sp in fr.lsd_order(eye):
        if used[sp]:
            continue
        reg = [int(sp)]
        used[sp] = True
        ra = ang[sp]
        sx, sy = np.float32(math.cos(ra)), np.float32(math.sin(ra))
        k = 0
        while k < len(reg):
            px, py = reg[k] % w, reg[k] // w
            k += 1
            for yy in range(max(py - 1, 0), min(py + 1, h - 1) + 1):
                for xx in range(max(px - 1, 0), min(px + 1, w - 1) + 1):
                    q = yy * w + xx
                    if used[q]:
                        continue
                    d = abs(ra - ang[q])
                    if d > 1.5 * math.pi:
                        d = abs(d - 2 * math.pi)
                    if d <= prec:
                        used[q] = True
                        reg.append(q)
                        sx = np.float32(sx + trig[q, 0])
                        sy = np.float32(sy + trig[q, 1])
                        ra = po.fast_atan2(float(sy), float(sx)) * (math.pi / 180)
        sizes.append(len(reg))
    return np.array(sizes), min_reg


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
    g.capi, g.Frontend, g.po = capi, Frontend, po
    g.frames = [np.stack([bars(0), bars(6)]), np.stack(synth.make_stereo_pair(90, W, H))]
    # the oracle, once: segments, tables and (the bars) the region sizes
    g.segs, g.want = [], []
    for f, pair in enumerate(g.frames):
        fr = po.Frame(po.Config.from_buffer_copy(bytes(config(g, 1))))
        out = {}
        for eye, k in ((0, "L"), (1, "R")):
            fr.orb_extract(eye, pair[eye])
            m, kl, ld = fr.line_extract(eye, pair[eye])
            out["kl" + k], out["ldesc" + k] = kl.tobytes(), np.asarray(ld).tobytes()
            g.segs.append(fr.lsd_segments(eye).copy())
            if f == 0 and eye == 0:
                g.sizes, g.min_reg = grower_sizes(po, fr, eye)
        fr.stereo_points()
        disp, le, _ = fr.stereo_lines()
        out["disp"], out["le"] = disp.tobytes(), le.tobytes()
        g.want.append(out)
    return g


def config(g, frames):
    return g.capi.default_config(W, H, orb_nfeatures=300, lsd_nfeatures=0, max_frames=frames)


def frontend(g, monkeypatch, mode, frames, debug):
    monkeypatch.delenv("PLI_TX_KEYS", raising=False)
    if mode == "ranks":
        monkeypatch.setenv("PLI_TX_KEYS", "0")
    fe = g.Frontend(config(g, frames), dev=mode == "ranks")       # (the product library does not read the switch)
    if debug:
        fe.debug_enable(True)
    return fe


def segments(fe, g, image):
    raw = fe.debug_fetch(image, g.capi.DBG_LSD_SEGMENTS)
    n = int(raw[:4].view(np.int32)[0])
    return raw[4:4 + 16 * n].view(np.float32).reshape(-1, 4)


def test_the_bars_give_every_size_on_the_oracle(gpu):
    g = gpu
    big = g.sizes[g.sizes >= g.min_reg]
    print("minRegSize %d, %d regions, %d of them large enough; sizes %s" % (g.min_reg, len(g.sizes), len(big), sorted(big.tolist())))
    assert len(big) == len(g.segs[0]), "the restated grower and the oracle disagree on the number of regions"
    assert g.min_reg <= min(SIZES)
    missing = [n for n in SIZES if n not in big]
    assert not missing, "no region of %s pixels: change the bars" % missing


@pytest.mark.parametrize("mode", ["keys", "ranks"])
def test_single_frames_segments_and_sizes(gpu, monkeypatch, mode):
    g = gpu
    fe = frontend(g, monkeypatch, mode, 1, debug=True)
    for f, pair in enumerate(g.frames):
        for eye in (0, 1):
            fe.line_extract(eye, pair[eye])
            got = segments(fe, g, eye)
            assert got.tobytes() == g.segs[2 * f + eye].tobytes(), "%s: segments of frame %d eye %d differ from the oracle" % (mode, f, eye)
            if f == 0 and eye == 0:
                # every region of at least minRegSize pixels went to region2rect (a debug context makes no short-segment cut)
                plane = fe.debug_fetch(eye, g.capi.DBG_LSD_SIZES).view(np.int32)
                reached = set(plane[plane >= g.min_reg].tolist())
                missing = [n for n in SIZES if n not in reached]
                print("%s: %d distinct sizes reached region2rect" % (mode, len(reached)))
                assert not missing, "%s: no region of %s pixels reached region2rect" % (mode, missing)
    assert fe.lsd_round_stats()[2] == 0                       # nobody on the sequential grower
    fe.close()


def assert_tables(g, rec, f, what):
    for k in TABLES:
        assert np.asarray(rec[k]).tobytes() == g.want[f][k], "%s: %s of frame %d differs from the oracle" % (what, k, f)


@pytest.mark.parametrize("mode", ["keys", "ranks"])
def test_line_tables_single_and_second_call(gpu, monkeypatch, mode):
    g = gpu
    for f, pair in enumerate(g.frames):                        # first calls of a context: rounds with looks
        fe = frontend(g, monkeypatch, mode, 1, debug=False)
        assert_tables(g, fe.batch_run_host(pair[None])[0], f, "%s, single frame" % mode)
        assert fe.lsd_round_stats()[2] == 0
        fe.close()
    fe = frontend(g, monkeypatch, mode, 2, debug=False)        # a batch called twice: the second call runs look-free rounds and the tail
    imgs = np.stack(g.frames)
    fe.batch_run_host(imgs)
    recs = fe.batch_run_host(imgs)
    for f in (0, 1):
        assert_tables(g, recs[f], f, "%s, batch, second call" % mode)
    assert fe.lsd_round_stats()[2] == 0
    fe.close()


@pytest.mark.parametrize("mode", ["keys", "ranks"])
def test_second_call_of_a_batch_lists_the_oracles_segments(gpu, monkeypatch, mode):
    g = gpu
    fe = frontend(g, monkeypatch, mode, 2, debug=True)
    imgs = np.stack(g.frames)
    fe.batch_run_host(imgs)
    fe.batch_run_host(imgs)
    stats = fe.lsd_round_stats()
    print("%s: round stats of the second call %s" % (mode, (stats,)))
    # (out[0]: -1 the persistent tail ran the late rounds, > 0 planned rounds, 0 the host looked; the tail starts at round 3 or 4)
    assert stats[0] != 0, "the second call was meant to run its rounds without a look"
    assert stats[1] >= 5, "the late rounds were meant to have work: the slowest image settled in round %d" % stats[1]
    assert stats[2] == 0
    for image in range(4):
        assert segments(fe, g, image).tobytes() == g.segs[image].tobytes(), "%s: segments of image %d differ from the oracle" % (mode, image)
    fe.close()
