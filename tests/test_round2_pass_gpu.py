"""Round 2's pass over the owner map (k_tx_round2, pli_slam_amd/csrc/lsd_tile.hip) on the smallest grids: the pass moves round 1's owner
words into the owner plane, finds the regions that are dead or lost a contested claim and gives their pixels their own ids back.
Whatever order it loads in and whichever blocks of 32 x 32 pixels its workgroups take (two forms that read less were measured and
are slower: profiles/lbd_round2_traffic_ab.json), nothing an integrator reads may change: every line table is the oracle's, byte for
byte, and nobody takes the device-side fallback.

Images whose scaled sizes give 1 x 1, 2 x 2 and 3 x 2 tiles of 64 x 64 (regions cross tile borders; 4, 12 and 24 blocks of 32 x 32 per
image), as single images and in batches of 1, 3 and 9 stereo frames: grids of fewer than 8 blocks, of a count that is no multiple of 8
(4, 12, 72 ...), and of many more.  Key mode (the product library) and rank mode (development build, PLI_TX_KEYS=0).  Every batch
holds a diagonal-stripes pair, the hostile image of test_gpu_parity.test_lsd_hostile_images: long regions with seeds in several
tiles, so round 1 leaves dead and contested regions for this pass to find."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (image size, lsd_scale) -> scaled size: 64 x 64 * 0.8 = 51 x 51; 100 x 70 * 1.2 = 120 x 84; 150 x 90 * 1.2 = 180 x 108
SHAPES = {"1x1": (64, 64, 0.8, (1, 1), 4), "2x2": (100, 70, 1.2, (2, 2), 12), "3x2": (150, 90, 1.2, (3, 2), 24)}
TABLES = ("klL", "klR", "ldescL", "ldescR", "disp", "le")


def stripes(W, H, phase=0):
    yy, xx = np.mgrid[0:H, 0:W]
    return ((np.sin((xx + 2 * yy + phase) / 5.0) * 0.5 + 0.5) * 255).astype(np.uint8)


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
    g.pairs, g.want = {}, {}
    return g


def config(g, shape, frames):
    W, H, scale, tiles, blocks = SHAPES[shape]
    # (the scaled size behind the tile and block counts this file is about)
    LW, LH = int(round(W * scale)), int(round(H * scale))
    assert ((LW + 63) // 64, (LH + 63) // 64) == tiles and ((LW + 31) // 32) * ((LH + 31) // 32) == blocks
    return g.capi.default_config(W, H, orb_nfeatures=100, lsd_nfeatures=0, lsd_scale=scale, max_frames=frames)


def pair(g, shape, i):
    """three distinct stereo pairs per shape: a crop of a synthetic scene, the stripes, another crop"""
    if (shape, i) not in g.pairs:
        W, H = SHAPES[shape][:2]
        if i == 1:
            g.pairs[(shape, i)] = (stripes(W, H), stripes(W, H, 3))
        else:                                                 # (a crop: the scene generator wants larger images)
            L, R = g.synth.make_stereo_pair(70 + i, 376, 240)
            g.pairs[(shape, i)] = (np.ascontiguousarray(L[60:60 + H, 100:100 + W]), np.ascontiguousarray(R[60:60 + H, 100:100 + W]))
    return g.pairs[(shape, i)]


def oracle_tables(g, shape, i):
    """the oracle's line tables of one pair, computed once and shared by the cases"""
    if (shape, i) not in g.want:
        cfg = config(g, shape, 1)
        fr = g.po.Frame(g.po.Config.from_buffer_copy(bytes(cfg)))
        out = {}
        for eye, img, k in ((0, pair(g, shape, i)[0], "L"), (1, pair(g, shape, i)[1], "R")):
            m, kl, ld = fr.line_extract(eye, img)
            out["kl" + k], out["ldesc" + k], out["n" + k] = kl.tobytes(), np.asarray(ld).tobytes(), m
        disp, le, _ = fr.stereo_lines()
        out["disp"], out["le"] = disp.tobytes(), le.tobytes()
        g.want[(shape, i)] = out
    return g.want[(shape, i)]


def test_the_images_have_lines(gpu):
    for shape in SHAPES:
        for i in range(3):
            w = oracle_tables(gpu, shape, i)
            assert w["nL"] + w["nR"] > 0, (shape, i)
    assert oracle_tables(gpu, "3x2", 1)["nL"] >= 4            # the stripes' flanks


@pytest.mark.parametrize("frames", [1, 3, 9])
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("mode", ["keys", "ranks"])
def test_every_table_is_the_oracles(gpu, monkeypatch, mode, shape, frames):
    g = gpu
    monkeypatch.delenv("PLI_TX_KEYS", raising=False)
    if mode == "ranks":
        monkeypatch.setenv("PLI_TX_KEYS", "0")
    dev = mode == "ranks"                                     # (the product library does not read the switch)
    stages = g.capi.RUN_LINES | g.capi.RUN_STEREO_LINES
    fe = g.Frontend(config(g, shape, frames), dev=dev)
    which = [(f + 1) % 3 for f in range(frames)]              # (frame 0 is the stripes pair)
    imgs = np.stack([np.stack(pair(g, shape, i)) for i in which])
    for call in range(2):                                     # (the second call runs its rounds without looks)
        recs = fe.batch_run_host(imgs, stages=stages)
        for f, i in enumerate(which):
            want = oracle_tables(g, shape, i)
            for k in TABLES:
                assert np.asarray(recs[f][k]).tobytes() == want[k], "%s, %s, %d frames, call %d, frame %d: %s" % (mode, shape, frames, call, f, k)
        assert fe.lsd_round_stats()[2] == 0, "an image took the device-side fallback"
    if frames == 1:
        # one image per launch: the smallest grids (4, 12, 24 blocks)
        for i in range(3):
            for eye, k in ((0, "L"), (1, "R")):
                n, kl, ld = fe.line_extract(eye, pair(g, shape, i)[eye])
                want = oracle_tables(g, shape, i)
                assert n == want["n" + k] and kl.tobytes() == want["kl" + k] and ld.tobytes() == want["ldesc" + k], (mode, shape, i, eye)
        assert fe.lsd_round_stats()[2] == 0
    fe.close()
