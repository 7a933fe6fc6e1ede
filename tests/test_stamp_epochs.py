"""One context, many LSD calls, different images in the same slots: what a call leaves in the context must not reach the next one.

The tile relaxation keeps two planes of ROUND STAMPS per image slot (rgDirty, rgLost: one word per region id).  They are not cleared
per call: a call stamps with `base + round`, and the base moves up with every call of the context past every round a call can write
(capi_host.hpp: pli_ctx::lineStampNext).  A stale stamp that matched a round of a later call would regrow or carry the wrong regions,
so every test here reuses ONE context for a sequence of calls whose images change under the slots — photographs and the hostile
images that need many rounds among them — and compares every call, byte for byte, with the table a FRESH context writes for the same
images, and one record per call with the oracle.

The sequences cover: the batch entry point with device pointers, the three product schedules (lsd_mode 0, 2, 3) with the persistent
tail kernel and with planned rounds (PLI_TX_TAIL=0), batch sizes and image slots that change between calls (a sub-range, the
single-frame entry point, the per-eye entry point, the two slots of the pipelined host entry point), the zeroing of the planes when the
base would overflow (dev switch PLI_TX_STAMP0), and the device-side sequential fallback after a call that left stamps (PLI_RX_PLAN).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, F = 752, 480, 4


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from pli_slam_amd import capi, realdata, synth
    from pli_slam_amd.frontend import Frontend
    from oracle import pyoracle as po

    class G:
        pass
    g = G()
    g.capi, g.synth, g.Frontend, g.po, g.realdata, g.torch = capi, synth, Frontend, po, realdata, torch
    return g


def image_pool(g):
    """Stereo pairs of 752 x 480: synthetic scenes, photographs, and the hostile images of test_lsd_hostile_images at full size (noise:
    hundreds of thousands of tiny regions; checkerboard, stripes: long regions over many tiles, i.e. many rounds)."""
    rng = np.random.default_rng(5)
    noise = rng.integers(0, 256, (H, W), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    checker = (((xx // 16) + (yy // 16)) % 2 * 200 + 20).astype(np.uint8)
    stripes = ((np.sin((xx + 2 * yy) / 5.0) * 0.5 + 0.5) * 255).astype(np.uint8)
    mixed = np.where(xx < W // 2, noise, stripes).astype(np.uint8)
    photos = g.realdata.frames_752x480(4, seed=3)
    synth = [g.synth.make_stereo_pair(70 + i, W, H) for i in range(3)]
    pool = [synth[0], photos[0], (stripes, checker), photos[1], synth[1], (mixed, noise), photos[2], (checker, mixed), synth[2],
            photos[3], (noise, stripes)]
    return [(np.ascontiguousarray(l), np.ascontiguousarray(r)) for l, r in pool]


def batch_of(pool, k, n=F):
    """Call k's frames: a window of the pool that moves by three, so that every slot sees another image in every call."""
    return [pool[(3 * k + i) % len(pool)] for i in range(n)]


def run_device(g, fe, frames):
    """pli_batch_run on device pointers; returns the table (host bytes)."""
    torch = g.torch
    imgs = np.stack([np.stack(f) for f in frames])
    n = len(frames)
    dimg = torch.from_numpy(imgs).cuda()
    dtab = torch.zeros(fe.table_bytes(n), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    fe.batch_run_device(n, dimg.data_ptr(), dimg.data_ptr() + W * H, W, 2 * W * H, dtab.data_ptr())
    fe.sync()
    return dtab.cpu().numpy().copy()


def fresh_table(g, cfg, frames, dev=False):
    fe = g.Frontend(cfg, dev=dev)
    try:
        return run_device(g, fe, frames)
    finally:
        fe.close()


def ocfg(g, cfg):
    return g.po.Config.from_buffer_copy(bytes(cfg))


def assert_frame_equal(g, rec, fr, L, R, what=""):
    from test_gpu_parity import assert_frame_equal as afe     # (inside the call, as tests/test_real_images.py borrows it)
    afe(g, rec, fr, L, R, what)


def check_call(g, cfg, fe, tab, frames, what, oracle_frame, dev=False):
    want = fresh_table(g, cfg, frames, dev=dev)
    assert tab.tobytes() == want.tobytes(), "%s: the reused context's table differs from a fresh context's" % what
    L, R = frames[oracle_frame]
    assert_frame_equal(g, fe.parse_record(tab, oracle_frame), g.po.Frame(ocfg(g, cfg)), L, R, what)


@pytest.mark.parametrize("mode,tail", [(0, None), (3, None), (2, None), (0, "0"), (3, "0")])
def test_consecutive_calls_with_other_images_in_the_same_slots(gpu, mode, tail, monkeypatch):
    """Nine calls on one context; call k + 1 finds call k's stamps under other pixels."""
    g = gpu
    if tail is not None:
        monkeypatch.setenv("PLI_TX_TAIL", tail)               # planned rounds instead of the persistent tail kernel
    cfg = g.capi.default_config(W, H, orb_nfeatures=600, lsd_nfeatures=0, max_frames=F, lsd_mode=mode)
    fe = g.Frontend(cfg, dev=False)
    pool = image_pool(g)
    for k in range(9):
        frames = batch_of(pool, k)
        tab = run_device(g, fe, frames)
        check_call(g, cfg, fe, tab, frames, "mode %d tail %s call %d" % (mode, tail, k), k % F, dev=False)
    if mode != 2:
        assert fe.lsd_round_stats()[2] == 0, fe.lsd_round_stats()      # (nobody took the sequential fallback on the way)


@pytest.mark.parametrize("mode", [0, 3])
def test_batch_size_and_image_slot_change_between_calls(gpu, mode):
    """Full batch, a sub-range, the single-frame entry point, the per-eye entry point on slot 1, the full batch again, and the two
    slots of the pipelined host entry point (image slots F .. 2F - 1 for every second batch)."""
    g = gpu
    cfg = g.capi.default_config(W, H, orb_nfeatures=600, lsd_nfeatures=0, max_frames=F, lsd_mode=mode)
    fe = g.Frontend(cfg, dev=False)
    pool = image_pool(g)
    k = 0
    for n in (F, 2, F, 1, F):
        frames = batch_of(pool, k, n)
        check_call(g, cfg, fe, run_device(g, fe, frames), frames, "mode %d: %d frames (call %d)" % (mode, n, k), n - 1)
        k += 1
    # the single-frame entry point between two batch calls
    L, R = pool[(3 * k + 1) % len(pool)]
    rec = fe.frame_extract(L, R)
    assert_frame_equal(g, rec, g.po.Frame(ocfg(g, cfg)), L, R, "pli_frame_extract between batches")
    frames = batch_of(pool, k + 1)
    check_call(g, cfg, fe, run_device(g, fe, frames), frames, "mode %d: batch after pli_frame_extract" % mode, 0)
    # the per-eye entry point: image slot 1 alone, over what the batch left there
    img = pool[5][1]
    n1, kl, ld = fe.line_extract(1, img)
    m1, okl, old = g.po.Frame(ocfg(g, cfg)).line_extract(1, img)
    assert n1 == m1 and kl.tobytes() == okl.tobytes() and np.array_equal(ld, old), "line_extract on slot 1 after a batch"
    frames = batch_of(pool, k + 2)
    check_call(g, cfg, fe, run_device(g, fe, frames), frames, "mode %d: batch after line_extract" % mode, 1)
    # three batches through the two slots of the pipelined host entry point
    batches = [batch_of(pool, k + 3 + b) for b in range(3)]
    want = [fresh_table(g, cfg, fr) for fr in batches]
    npx = W * H
    lefts = [fe.pinned(F * npx).reshape(F, npx) for _ in range(3)]
    rights = [fe.pinned(F * npx).reshape(F, npx) for _ in range(3)]
    tabs = [fe.pinned(fe.table_bytes(F)) for _ in range(3)]
    for b, fr in enumerate(batches):
        lefts[b][:] = np.stack([f[0] for f in fr]).reshape(F, npx)
        rights[b][:] = np.stack([f[1] for f in fr]).reshape(F, npx)
        tabs[b][:] = 0xEE
    for b in range(3):
        fe.host_submit(F, lefts[b], rights[b], tabs[b])
    fe.host_wait_all()
    for b in range(3):
        assert np.asarray(tabs[b]).tobytes() == want[b].tobytes(), "pipelined host batch %d" % b
    frames = batch_of(pool, k + 6)
    check_call(g, cfg, fe, run_device(g, fe, frames), frames, "mode %d: batch after the pipelined batches" % mode, 2)


@pytest.mark.parametrize("tail", [None, "0"])
def test_the_stamp_base_overflow_zeroes_the_planes_between_two_calls(gpu, tail, monkeypatch):
    """Development library: the base starts 100 below INT_MAX (PLI_TX_STAMP0).  The first call of a context moves it by 97 in either
    schedule (the persistent tail and the first, host-watched call of the planned-rounds schedule both allow 96 rounds), which leaves
    3: the SECOND call, whatever it plans, would pass INT_MAX, so it zeroes both planes and starts again at 0 — over the stamps of call
    one, which sit just below INT_MAX.  Calls three to six then run on small bases.  Every call equals the fresh context's (which
    starts at 0: the switch is read when a context is created)."""
    g = gpu
    if tail is not None:
        monkeypatch.setenv("PLI_TX_TAIL", tail)
    cfg = g.capi.default_config(W, H, orb_nfeatures=600, lsd_nfeatures=0, max_frames=F, lsd_mode=3)
    monkeypatch.setenv("PLI_TX_STAMP0", str(2 ** 31 - 1 - 100))
    fe = g.Frontend(cfg, dev=True)
    monkeypatch.delenv("PLI_TX_STAMP0")
    pool = image_pool(g)
    for k in range(6):
        frames = batch_of(pool, k + 2)
        tab = run_device(g, fe, frames)
        check_call(g, cfg, fe, tab, frames, "overflow sequence, tail %s, call %d" % (tail, k), (k + 1) % F, dev=True)
    assert fe.lsd_round_stats()[2] == 0, fe.lsd_round_stats()


def test_the_sequential_fallback_after_a_call_that_left_stamps(gpu, monkeypatch):
    """Development library: two ordinary calls (hostile images: stamps of many rounds), then other images with a plan that is too
    short (PLI_RX_PLAN=3): the images that have not settled go to the device-side sequential grower; then an ordinary call again.
    All of them the oracle's, byte for byte."""
    g = gpu
    cfg = g.capi.default_config(W, H, orb_nfeatures=600, lsd_nfeatures=0, max_frames=F, lsd_mode=3)
    fe = g.Frontend(cfg, dev=True)
    pool = image_pool(g)
    for k in (0, 1):
        if k == 1:
            monkeypatch.setenv("PLI_TX_TAIL", "0")            # (planned rounds: the host learns how many rounds a call needs, the plan below applies)
        frames = batch_of(pool, k)
        check_call(g, cfg, fe, run_device(g, fe, frames), frames, "before the fallback, call %d" % k, 2, dev=True)
    monkeypatch.delenv("PLI_TX_TAIL")
    monkeypatch.setenv("PLI_RX_PLAN", "3")
    frames = batch_of(pool, 2)
    short = run_device(g, fe, frames)
    st = fe.lsd_round_stats()
    assert st[0] == 3 and st[2] >= 1, st                     # (three rounds planned, at least one image redone sequentially)
    monkeypatch.delenv("PLI_RX_PLAN")
    for f, (L, R) in enumerate(frames):
        assert_frame_equal(g, fe.parse_record(short, f), g.po.Frame(ocfg(g, cfg)), L, R, "fallback frame %d" % f)
    frames = batch_of(pool, 3)
    check_call(g, cfg, fe, run_device(g, fe, frames), frames, "after the fallback", 1, dev=True)
