"""pli_slam_amd.frontend.pack_keyframes: the flat tables (offsets + one contiguous array per column) that the four searches against
a batch of keyframes hand to the library.  No device, no library."""
import numpy as np
import pytest

from pli_slam_amd.capi import KEYPOINT_DT
from pli_slam_amd.frontend import BOW_COLUMNS, FUSE_COLUMNS, TRI_COLUMNS, pack_keyframes


def bow_kf(rng, n):
    return (rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.uniform(0, 360, n).astype(np.float32),
            rng.integers(-1, 9, n).astype(np.int32), rng.integers(0, 2, n).astype(np.uint8))


@pytest.mark.parametrize("spec", [BOW_COLUMNS, TRI_COLUMNS, FUSE_COLUMNS])
def test_an_empty_list(spec):
    off, cols = pack_keyframes([], spec, "x")
    assert off.dtype == np.int32 and off.tolist() == [0]
    assert len(cols) == len(spec)
    for col, (_, dt, tail) in zip(cols, spec):
        assert col.dtype == np.dtype(dt) and col.shape == (0,) + tuple(tail) and col.flags.c_contiguous


def test_an_empty_keyframe_in_the_middle_and_at_the_ends():
    rng = np.random.default_rng(0)
    kfs = [bow_kf(rng, n) for n in (0, 5, 0, 3, 0)]
    off, cols = pack_keyframes(kfs, BOW_COLUMNS, "x")
    assert off.dtype == np.int32 and off.tolist() == [0, 0, 5, 5, 8, 8]
    for c, (col, (_, dt, tail)) in enumerate(zip(cols, BOW_COLUMNS)):
        assert col.dtype == np.dtype(dt) and col.shape == (8,) + tuple(tail) and col.flags.c_contiguous
        for k, kf in enumerate(kfs):
            assert np.array_equal(col[off[k]:off[k + 1]], kf[c])
    off, cols = pack_keyframes([bow_kf(rng, 0)] * 3, BOW_COLUMNS, "x")
    assert off.tolist() == [0, 0, 0, 0] and cols[0].shape == (0, 32)


def test_a_column_one_short_raises():
    rng = np.random.default_rng(1)
    good, bad = bow_kf(rng, 4), bow_kf(rng, 6)
    bad = (bad[0], bad[1][:-1], bad[2], bad[3])                  # the angle column is one short
    with pytest.raises(ValueError, match="one angle, node and valid flag"):
        pack_keyframes([good, bad], BOW_COLUMNS, "every keyframe needs one angle, node and valid flag per descriptor")
    longer = (good[0], np.append(good[1], np.float32(1)), good[2], good[3])       # (the totals agree: it is per keyframe)
    with pytest.raises(ValueError):
        pack_keyframes([longer, bad], BOW_COLUMNS, "x")


def test_columns_are_converted_and_contiguous():
    rng = np.random.default_rng(2)
    kp = np.zeros(7, KEYPOINT_DT)
    kp["octave"] = np.arange(7)
    desc = rng.integers(0, 256, (7, 64), dtype=np.uint8)[:, ::2]  # not contiguous
    kf = (kp[::-1], desc, list(range(7)), [1] * 7, np.ones(7, bool), "F12", "ep")   # lists, bools, extra entries
    off, (k, d, n, m, s) = pack_keyframes([kf, kf], TRI_COLUMNS, "x")
    assert off.tolist() == [0, 7, 14]
    for col in (k, d, n, m, s):
        assert col.flags.c_contiguous and len(col) == 14
    assert k.dtype == KEYPOINT_DT and k["octave"][:7].tolist() == list(range(6, -1, -1))
    assert d.dtype == np.uint8 and np.array_equal(d[7:], desc)
    assert n.dtype == np.int32 and m.dtype == np.uint8 and s.dtype == np.uint8 and s.sum() == 14
    flat = pack_keyframes([(desc.reshape(-1), np.zeros(7), np.zeros(7), np.zeros(7))], BOW_COLUMNS, "x")[1]
    assert flat[0].shape == (7, 32) and flat[1].dtype == np.float32   # a flat descriptor buffer is n x 32
