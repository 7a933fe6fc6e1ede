"""The short-segment cut on the GPU (pli_slam_amd/csrc/common.hpp "SHORT-SEGMENT CUT"): the tile relaxation computes no segment for a
region whose bounding box says that the segment cannot pass the key-line length test, and the emit kernels drop such a region by the
same test.  Nothing an integrator reads may change: every table stays the oracle's, byte for byte, for every minimum length, in
key mode (the product library) and in rank mode (development build, PLI_TX_KEYS=0), on single frames and on batches whose second call
runs its rounds without looks; a debug context still lists every segment, a plain one a subsequence of them."""
import numpy as np
import pytest

from helpers_line_ref import bars_image, clamp_segments, lengths_of

pytestmark = pytest.mark.gpu

W, H = 376, 240
MLLS = (0.0, 0.025, 0.05, 0.2)
TABLES = ("klL", "klR", "ldescL", "ldescR", "disp", "le")


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
    g.pairs = {s: synth.make_stereo_pair(s, W, H) for s in (90, 91, 92)}
    g.want = {}
    return g


def config(g, mll, frames=3):
    return g.capi.default_config(W, H, orb_nfeatures=300, lsd_nfeatures=0, min_line_length=mll, max_frames=frames)


def oracle_tables(g, mll, seed):
    """the oracle's line tables of one synthetic pair, computed once per (minimum length, seed) and shared"""
    if (mll, seed) not in g.want:
        cfg = config(g, mll)
        fr = g.po.Frame(g.po.Config.from_buffer_copy(bytes(cfg)))
        L, R = g.pairs[seed]
        out = {}
        for eye, img, k in ((0, L, "L"), (1, R, "R")):
            fr.orb_extract(eye, img)
            m, kl, ld = fr.line_extract(eye, img)
            out["kl" + k], out["ldesc" + k] = kl.tobytes(), np.asarray(ld).tobytes()
        fr.stereo_points()
        disp, le, _ = fr.stereo_lines()
        out["disp"], out["le"] = disp.tobytes(), le.tobytes()
        out["nL"] = len(kl)
        g.want[(mll, seed)] = out
    return g.want[(mll, seed)]


def assert_tables(g, rec, mll, seed, what):
    want = oracle_tables(g, mll, seed)
    for k in TABLES:
        assert np.asarray(rec[k]).tobytes() == want[k], "%s: %s differs from the oracle (min_line_length %g, seed %d)" % (what, k, mll, seed)


@pytest.mark.parametrize("mll", MLLS)
@pytest.mark.parametrize("mode", ["keys", "ranks"])
def test_every_table_is_the_oracles(gpu, monkeypatch, mode, mll):
    g = gpu
    monkeypatch.delenv("PLI_TX_KEYS", raising=False)
    if mode == "ranks":
        monkeypatch.setenv("PLI_TX_KEYS", "0")
    dev = mode == "ranks"                                     # (the product library does not read the switch)
    import ctypes as C
    cut = int(g.capi.lib().pli_lsd_segment_box_cut(C.byref(config(g, mll))))
    assert (cut == -1) == (mll == 0.0)
    # single frames, first calls of a context: rounds with looks
    for seed in (90, 91):
        fe = g.Frontend(config(g, mll), dev=dev)
        rec = fe.batch_run_host(np.stack(g.pairs[seed])[None])[0]
        assert_tables(g, rec, mll, seed, "%s, single frame" % mode)
        assert fe.lsd_round_stats()[2] == 0                   # nobody on the sequential grower: the relaxation's tables
        fe.close()
    # a batch of three, called twice: the second call runs look-free rounds and the tail
    fe = g.Frontend(config(g, mll), dev=dev)
    imgs = np.stack([np.stack(g.pairs[s]) for s in (90, 91, 92)])
    fe.batch_run_host(imgs)
    recs = fe.batch_run_host(imgs)
    for f, seed in enumerate((90, 91, 92)):
        assert_tables(g, recs[f], mll, seed, "%s, batch frame %d, second call" % (mode, f))
    assert fe.lsd_round_stats()[2] == 0
    assert oracle_tables(g, 0.0, 90)["nL"] > oracle_tables(g, 0.05, 90)["nL"] > oracle_tables(g, 0.2, 90)["nL"]
    fe.close()


def segments(fe, g, eye, img):
    fe.line_extract(eye, img)
    raw = fe.debug_fetch(eye, g.capi.DBG_LSD_SEGMENTS)
    n = int(raw[:4].view(np.int32)[0])
    return raw[4:4 + 16 * n].view(np.float32).reshape(-1, 4).copy()


def test_plain_context_lists_a_subsequence_of_the_debug_contexts_segments(gpu):
    g = gpu
    for mll in (0.05, 0.0):
        cfg = config(g, mll, frames=1)
        plain, dbg = g.Frontend(cfg, dev=False), g.Frontend(cfg, dev=False)
        dbg.debug_enable(True)
        for eye, img in enumerate(g.pairs[90]):
            every = segments(dbg, g, eye, img)
            fr = g.po.Frame(g.po.Config.from_buffer_copy(bytes(cfg)))
            fr.line_extract(eye, img)
            assert np.array_equal(every, fr.lsd_segments(eye))            # the debug context: every detected segment
            some = segments(plain, g, eye, img)
            if mll == 0.0:
                assert np.array_equal(some, every)
                continue
            # in order, and nothing that is not there
            at, kept = 0, np.zeros(len(every), bool)
            for s in some:
                while at < len(every) and every[at].tobytes() != s.tobytes():
                    at += 1
                assert at < len(every), "a segment of the plain context is not in the debug context's list, or out of order"
                kept[at] = True
                at += 1
            e, _ = clamp_segments(every[~kept], W, H)
            gone = lengths_of(e)
            print("eye %d: %d of %d segments omitted, the longest %.3f px" % (eye, len(gone), len(every), gone.max(initial=0)))
            assert gone.max(initial=0) <= 12.0                              # nothing that passes `length > 12`
            assert 2 * len(gone) >= len(every), "the cut is not active: %d of %d omitted" % (len(gone), len(every))
            # ... and the switch follows pli_debug_enable both ways on one context
            dbg.debug_enable(False)
            assert np.array_equal(segments(dbg, g, eye, img), some)
            dbg.debug_enable(True)
        plain.close()
        dbg.close()


def test_bars_either_side_of_the_cut(gpu):
    """Noise-free bars one and two pixels either side of the length at which their edges pass the 12 px minimum: a bar of n pixels
    gives six segments of about (n + 1) / 1.2 px (the oracle: 10.0-10.8, 11.67-11.68, 12.50-12.51, 13.3 px for n = 12 .. 15), whose
    regions span n + 1 scaled pixels — 14^2 = 196 (cut) for n = 13 and 15^2 = 225 (kept) for n = 14, around the cut value 207."""
    g = gpu
    cfg = config(g, 0.05, frames=1)
    fe = g.Frontend(cfg, dev=False)
    counts = []
    for n in (12, 13, 14, 15):
        img = bars_image(W, H, 60, 60 + n, (40, 90, 150), 6)
        img[200:206, 100:300] = 200                                          # (a long bar: the tables are never empty)
        fr = g.po.Frame(g.po.Config.from_buffer_copy(bytes(cfg)))
        m, kl, ld = fr.line_extract(0, img)
        gn, gkl, gld = fe.line_extract(0, img)
        assert gn == m and gkl.tobytes() == kl.tobytes() and np.array_equal(gld, ld), "bars of %d px" % n
        counts.append(m)
    print("key lines for bars of 12..15 px:", counts)
    assert counts == [2, 2, 8, 8], "the bars were meant to straddle the cut (the long bar's two edges, then the six of the bars): %s" % counts
    fe.close()
