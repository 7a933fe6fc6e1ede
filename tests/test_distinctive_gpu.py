"""pli_distinctive_descriptors on the device (k_distinctive_wave, k_distinctive_block, k_distinctive_pick) through Frontend and the raw C ABI: best,
best_median and row_median of every group equal the restatement of MapPoint.cc:330-359 and the independent definition of
tests/helpers_distinctive.py exactly, at the wave, workgroup and size-class edges, for empty groups and calls, optional outputs,
misaligned tables, the cap and bad offsets."""
import numpy as np
import pytest

import helpers_distinctive as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from pli_slam_amd import capi
    from pli_slam_amd.frontend import Frontend
    fe = Frontend(capi.default_config(128, 96, orb_nfeatures=100, lsd_nfeatures=0))
    yield fe
    fe.close()


def check(fe, groups, fns=(H.restated_point, H.independent)):
    got = fe.distinctive_descriptors(groups)
    for fn in fns:
        want = H.expected(groups, fn)
        for g, w, what in zip(got, want, ("best", "best_median", "row_median")):
            assert g.dtype == w.dtype and np.array_equal(g, w), (fn.__name__, what, np.flatnonzero(g != w)[:8] if g.shape == w.shape else g.shape)
    return got


def raw(fe, desc, off, nfeat, best, best_median, row_median):
    """The C entry itself; every table a numpy array or None."""
    from pli_slam_amd.capi import ptr
    return fe.L.pli_distinctive_descriptors(fe.h, ptr(desc), ptr(off), nfeat, ptr(best), ptr(best_median), ptr(row_median))


def pack(groups):
    off = np.zeros(len(groups) + 1, np.int32)
    off[1:] = np.cumsum([len(g) for g in groups])
    desc = np.ascontiguousarray(np.concatenate([np.asarray(g, np.uint8).reshape(-1, 32) for g in groups]) if groups else np.zeros((0, 32), np.uint8))
    return desc, off


def test_mixed_sizes_in_one_call(gpu):
    """Both classes' wave and workgroup edges and the class split inside one `off`; empty groups first, in the middle and last."""
    rng = np.random.default_rng(11)
    sizes = [1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 0]
    rng.shuffle(sizes)
    sizes = [0] + sizes[:8] + [0] + sizes[8:] + [0]
    groups = [H.track(rng, n, float(rng.choice([0.05, 0.15, 0.5]))) for n in sizes]
    best, _, _ = check(gpu, groups)
    assert (best > 0).sum() >= 5


def test_many_small_groups(gpu):
    """The LocalMapping shape: more wave-groups than one pass of the grid."""
    rng = np.random.default_rng(12)
    groups = [H.track(rng, int(rng.integers(2, 13)), 0.15) for _ in range(3000)]
    best, _, _ = check(gpu, groups)
    assert (best > 0).sum() > 1000


def test_hand_groups(gpu):
    hg = H.hand_groups()
    names = sorted(hg)
    groups = [hg[n][0] for n in names] + [H.complement_pairs(64), H.complement_pairs(65)]
    best, bm, rows = check(gpu, groups)
    at = 0
    for p, n in enumerate(names):
        b, m, med = hg[n][1]
        assert (int(best[p]), int(bm[p]), rows[at:at + len(med)].tolist()) == (b, m, med), n
        at += len(med)
    # 64 rows: 32 copies of a and 32 of ~a, median index 31 -> 0 for every row; 65 rows: 33 of a (median index 32 -> 0), 32 of ~a (-> 256)
    assert rows[at:at + 64].tolist() == [0] * 64 and rows[at + 64:].tolist() == [0, 256] * 32 + [0]
    assert best[-2:].tolist() == [0, 0] and bm[-2:].tolist() == [0, 0]


@pytest.mark.parametrize("n", [1024, 1025, 2048])
def test_long_groups(gpu, n):
    """Long groups between two of the small class, up to the cap (64 KiB of descriptors in LDS)."""
    rng = np.random.default_rng(n)
    best, _, _ = check(gpu, [H.track(rng, 70, 0.15), H.track(rng, n, 0.15), H.track(rng, 9, 0.5)], fns=(H.independent,))
    assert best[1] > 0


def test_over_the_cap_writes_nothing(gpu):
    from pli_slam_amd import capi
    rng = np.random.default_rng(13)
    desc, off = pack([H.track(rng, 5, 0.1), rng.integers(0, 256, (capi.DISTINCTIVE_MAX_OBS + 1, 32), dtype=np.uint8)])
    best = np.full(2, 77, np.int32); bm = np.full(2, 78, np.int32); rows = np.full(int(off[-1]), 79, np.int32)
    assert raw(gpu, desc, off, 2, best, bm, rows) == -3        # PLI_ERR_CAPACITY
    assert (best == 77).all() and (bm == 78).all() and (rows == 79).all()


def test_bad_offsets(gpu):
    rng = np.random.default_rng(14)
    desc = rng.integers(0, 256, (10, 32), dtype=np.uint8)
    best = np.full(2, 77, np.int32)
    for off in ([1, 4, 10], [0, 6, 4]):
        assert raw(gpu, desc, np.array(off, np.int32), 2, best, None, None) == -1      # PLI_ERR_INVALID
    assert raw(gpu, None, np.array([0, 4, 10], np.int32), 2, best, None, None) == -1
    assert (best == 77).all()
    with pytest.raises(capi_error()):
        gpu.distinctive_descriptors([rng.integers(0, 256, (2049, 32), dtype=np.uint8)])


def capi_error():
    from pli_slam_amd import capi
    return capi.PliError


def test_optional_outputs(gpu):
    rng = np.random.default_rng(15)
    groups = [H.track(rng, n, 0.15) for n in (7, 0, 80, 33)]
    desc, off = pack(groups)
    want = H.expected(groups)
    for with_bm, with_rows in ((True, True), (True, False), (False, True), (False, False)):
        best = np.full(4, 77, np.int32)
        bm = np.full(4, 78, np.int32) if with_bm else None
        rows = np.full(int(off[-1]), 79, np.int32) if with_rows else None
        assert raw(gpu, desc, off, 4, best, bm, rows) == 0
        assert np.array_equal(best, want[0])
        assert bm is None or np.array_equal(bm, want[1])
        assert rows is None or np.array_equal(rows, want[2])


def test_empty_calls(gpu):
    best, bm, rows = gpu.distinctive_descriptors([])
    assert len(best) == 0 and len(bm) == 0 and len(rows) == 0
    assert raw(gpu, None, np.zeros(1, np.int32), 0, None, None, None) == 0
    best, bm, rows = gpu.distinctive_descriptors([np.zeros((0, 32), np.uint8)] * 3)
    assert best.tolist() == [-1] * 3 and bm.tolist() == [H.INT_MAX] * 3 and len(rows) == 0
    b = np.full(3, 77, np.int32)
    assert raw(gpu, None, np.zeros(4, np.int32), 3, b, None, None) == 0 and b.tolist() == [-1] * 3


def test_tables_one_byte_off_alignment(gpu):
    rng = np.random.default_rng(16)
    groups = [H.track(rng, n, 0.15) for n in (5, 64, 70, 12)]
    desc, off = pack(groups)
    want = H.expected(groups)

    def shifted(a):
        buf = np.zeros(a.nbytes + 1, np.uint8)
        buf[1:] = a.view(np.uint8).reshape(-1)
        v = buf[1:].view(a.dtype).reshape(a.shape)
        assert v.ctypes.data % 2 == 1
        return v

    best, bm, rows = (shifted(np.zeros(n, np.int32)) for n in (4, 4, int(off[-1])))
    assert raw(gpu, shifted(desc), shifted(off), 4, best, bm, rows) == 0
    assert np.array_equal(best, want[0]) and np.array_equal(bm, want[1]) and np.array_equal(rows, want[2])


def test_scratch_reuse_across_calls(gpu):
    rng = np.random.default_rng(17)
    for sizes in ([200, 30, 90, 5] * 5, [4, 6], [130, 3, 260, 64] * 6):
        check(gpu, [H.track(rng, n, 0.15) for n in sizes], fns=(H.independent,))
