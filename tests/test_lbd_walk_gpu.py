"""k_lbd's walk in blocks (pli_slam_amd/csrc/line_kernels.hip): a lane computes the clamped coordinates of 32 steps of its row of the
line support region, issues their gathers together and sums behind them; the last block of a row ends at a bound, a remainder of up
to 16 steps takes the half block.  Only the order in which the loads are issued differs from the reference's loop, so the 72 floats
and the 32 descriptor bytes of every key line must be the oracle's, bit for bit — in particular for lines whose pixel count sits on,
one below and one above a multiple of the block (31, 32, 33, 63, 64, 65), either side of the half block's bound (16, 17, 48, 49)
and for a line of more than four blocks, and for rows that leave the image on every side.

Small images (160 x 120), one soft-edged bright bar each: at 0, 90, 45, 135 degrees and two shallow angles, starting within a few
pixels of a border (the 63-row support band and the first steps of the rows are clamped), lengths swept so that every class occurs.
The sweep is checked on the CPU oracle first: a class without a key line is an error of this file, not a reason to skip."""
import numpy as np
import pytest

W, H = 160, 120
CLASSES = (31, 32, 33, 63, 64, 65, 16, 17, 48, 49)
ANGLES = (0, 90, 45, 135, 7, 83)


def bar_image(deg, length, where, half=2.0, lo=40, hi=210):
    """a bright bar of `length` px along `deg` (image coordinates, y down), 2 * half px thick with soft edges, from a start point a few
    pixels from two borders; `where` picks the corner"""
    if deg in (0, 7):
        x0, y0 = (8, 30) if where == 0 or length > 100 else (8, H - 14 - (8 if deg else 0))
    elif deg in (90, 83):
        x0, y0 = (30, 4) if where == 0 or length > 80 else (W - 20, 4)
    elif deg == 45:
        x0, y0 = 6, 6
    else:
        x0, y0 = W - 10, 6
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    t = (xx - x0) * c + (yy - y0) * s
    d = np.abs(-(xx - x0) * s + (yy - y0) * c)
    a = np.clip(half + 0.5 - d, 0, 1) * np.clip(np.minimum(t + 0.5, length + 0.5 - t), 0, 1)
    return (lo + (hi - lo) * a).astype(np.uint8)


def lengths_for(deg):
    """bar lengths whose key lines have pixel counts around 32 and 64 (a diagonal line of L px has about L / sqrt 2 + 1 pixels)"""
    if deg in (45, 135):
        return list(range(40, 50)) + list(range(85, 96))
    if deg in (0, 90):
        return list(range(13, 20)) + list(range(28, 37)) + list(range(45, 52)) + list(range(59, 68))
    return list(range(28, 37)) + list(range(59, 68))


def all_images():
    out = []
    for deg in ANGLES:
        for i, L in enumerate(lengths_for(deg)):
            out.append((deg, L, bar_image(deg, L, i & 1)))
    out.append((0, 140, bar_image(0, 140, 0)))            # more than four blocks
    out.append((7, 140, bar_image(7, 140, 0)))
    return out


@pytest.fixture(scope="module")
def corpus():
    """the images and the oracle's key lines, floats and descriptors, computed once"""
    import torch  # noqa: F401  (before the library, as in every GPU test of the suite: one HIP runtime per process, the one torch loads)
    from pli_slam_amd import capi
    from oracle import pyoracle as po
    cfg = capi.default_config(W, H, orb_nfeatures=100, lsd_nfeatures=0, max_frames=1)
    rows = []
    for n, (deg, L, img) in enumerate(all_images()):
        eye = n & 1
        fr = po.Frame(po.Config.from_buffer_copy(bytes(cfg)))
        m, kl, ld = fr.line_extract(eye, img)
        rows.append(dict(deg=deg, L=L, eye=eye, img=img, m=m, kl=kl, ld=np.asarray(ld), lf=np.asarray(fr.lbd_float(eye, m))))
    return cfg, rows


def test_the_bars_give_every_length_class(corpus):
    """CPU: the oracle alone yields a key line in every class, at least one longer than four blocks, and at every angle"""
    cfg, rows = corpus
    have = {}
    for r in rows:
        for k in r["kl"]["numOfPixels"]:
            have.setdefault(int(k), set()).add(r["deg"])
    print("pixel counts of the corpus:", sorted(have))
    for c in CLASSES:
        assert c in have, "no key line of %d pixels in the corpus: adjust lengths_for()" % c
    assert max(have) > 4 * 32
    for deg in ANGLES:
        got = sorted(k for k in have if deg in have[k])
        assert any(k >= 31 for k in got), "no line of a block or more at %d degrees" % deg
    # ... and lines of a block or more come within 31 px of each border: the rows of their support bands are clamped on every side
    long = np.concatenate([r["kl"][r["kl"]["numOfPixels"] >= 31] for r in rows])
    xs = np.concatenate([long["startPointX"], long["endPointX"]])
    ys = np.concatenate([long["startPointY"], long["endPointY"]])
    assert xs.min() < 31 and ys.min() < 31 and xs.max() > W - 1 - 31 and ys.max() > H - 1 - 31, (xs.min(), ys.min(), xs.max(), ys.max())


@pytest.mark.gpu
def test_floats_and_descriptors_are_the_oracles(corpus):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from pli_slam_amd import capi
    from pli_slam_amd.frontend import Frontend
    cfg, rows = corpus
    dbg, plain = Frontend(cfg), Frontend(cfg)
    dbg.debug_enable(True)
    seen = set()
    for r in rows:
        what = "%d degrees, %d px, eye %d" % (r["deg"], r["L"], r["eye"])
        for fe in (dbg, plain):
            n, kl, ld = fe.line_extract(r["eye"], r["img"])
            assert n == r["m"] and kl.tobytes() == r["kl"].tobytes(), what
            assert np.array_equal(ld, r["ld"]), what + ": descriptor bytes"
        lf = dbg.debug_fetch(r["eye"], capi.DBG_LBD_FLOAT).view(np.float32).reshape(-1, 72)[:r["m"]]
        assert np.array_equal(lf, r["lf"]), what + ": the 72 floats"
        seen.update(int(k) for k in r["kl"]["numOfPixels"])
    assert set(CLASSES) <= seen
    dbg.close()
    plain.close()
