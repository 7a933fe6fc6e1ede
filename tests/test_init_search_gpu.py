"""pli_search_for_initialization on the MI355X (the product library): monocular initialisation's
ORBmatcher::SearchForInitialization (ORBmatcher.cc:706-821) equals the Python restatements of tests/test_init_search_cpu.py exactly
(raw12, matches12, nmatches and the updated vbPrevMatched).  That file shows, on the CPU, that the constructed scene takes every
exit of the reference's loops (evictions, left-out candidates, ratio rejections, filtered and already evicted histogram entries),
so the equalities here are not vacuous."""
import ctypes as C

import numpy as np
import pytest

from pli_slam_amd import capi, realdata, synth
from test_fuse_search_gpu import stereo_frame
from test_init_search_cpu import (BOUNDS, SCENE_SEED, chain_scene, dist_limit, hand_cases, init_candidates, init_search_fast,
                                  init_search_scalar, keypoints, points_of, scene, table, wrap360)

pytestmark = pytest.mark.gpu
W, H = 752, 480
NLEVELS = 8
CAP = 8192                                                # PLI_BOW_MAX_FEATURES
LIST_WIDTH = 16                                           # the candidate list of one i1 (INIT_LIST_WIDTH, match_capi.hip)


@pytest.fixture(scope="module")
def fe():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from pli_slam_amd.frontend import Frontend
    f = Frontend(capi.default_config(W, H), dev=False)
    assert f.cfg.orb_nlevels == NLEVELS
    yield f
    f.close()


def call(fe, t1, t2, prev=None, bounds=BOUNDS, window=100, nnratio=0.9, check_ori=True):
    prev = points_of(t1) if prev is None else prev
    return fe.search_for_initialization(keypoints(t1), t1.desc, prev, keypoints(t2), t2.desc, bounds, window, nnratio, check_ori)


def check(fe, t1, t2, prev=None, scalar=False, **kw):
    prev = points_of(t1) if prev is None else np.asarray(prev, np.float32)
    before = prev.copy()
    nm, m12, raw, new_prev = call(fe, t1, t2, prev, **kw)
    assert prev.tobytes() == before.tobytes()                                 # prev_matched is not written
    kw = dict(kw)
    kw["check_ori"] = kw.pop("check_ori", True)
    wr, wm, wn, wp = (init_search_scalar if scalar else init_search_fast)(t1, t2, prev, **kw)
    assert np.array_equal(raw, wr), "%d of %d raw12 differ" % (int((raw != wr).sum()), len(wr))
    assert np.array_equal(m12, wm), "%d of %d matches12 differ" % (int((m12 != wm).sum()), len(wm))
    assert nm == wn and new_prev.tobytes() == wp.tobytes()
    return nm, m12, raw, new_prev


@pytest.mark.parametrize("check_ori", [True, False])
def test_constructed_scene(fe, check_ori):
    t1, (t2, _, _) = scene(np.random.default_rng(SCENE_SEED))
    nm, m12, raw, _ = check(fe, t1, t2, window=100, nnratio=0.9, check_ori=check_ori, scalar=True)
    print("check_orientation %d: %d matches after the walk, %d returned" % (check_ori, int((raw >= 0).sum()), nm))
    assert int((raw >= 0).sum()) == 141 and nm == (111 if check_ori else 141)           # the figures of the CPU file's docstring
    for window, nnratio in ((0, 0.9), (15, 0.6), (100, 3.0), (100, 0.1)):                # 0.1: the lists hold every distance
        check(fe, t1, t2, window=window, nnratio=nnratio, check_ori=check_ori)
    check(fe, t1, t2, bounds=(10.0, 700.0, 20.0, 470.0), check_ori=check_ori)           # keypoints outside the grid


def test_hand_worked_cases(fe):
    for name, (t1, t2, prev, kw, raw, m12, nm) in hand_cases().items():
        n, m, r, _ = check(fe, t1, t2, prev, scalar=True, **kw)
        assert (r.tolist(), m.tolist(), n) == (raw, m12, nm), name
    t1, t2, _, kw, raw, _, _ = hand_cases()["histogram_counts_evicted"]
    n, m, r, _ = check(fe, t1, t2, check_ori=False, **kw)
    assert r.tolist() == raw and m.tolist() == raw and n == 7


def test_a_chain_of_three_calls(fe):
    """F1 against F2, F3 and F4 with vbPrevMatched carried as Tracking.cc does, from the device's own results."""
    t1, frames = chain_scene()
    prev = points_of(t1)
    counts = []
    for t in frames:
        nm, _, _, prev = check(fe, t1, t, prev, window=100)
        counts.append(nm)
    assert min(counts) > 30
    alone = call(fe, t1, frames[2], points_of(t1), window=100)[0]             # the carried windows matter
    assert alone < counts[2]


def crowded(rng, nspots=12, per1=12, per2=18):
    """Every spot holds per2 F2 keypoints at the distinct small distances 0, 3, .. 3 * (per2 - 1) from the spot's descriptor and
    per1 F1 keypoints at most one bit away from it: each window holds more candidates within the limit (55) than the list is wide,
    and the F1 keypoints of a spot take, lose and retake rows."""
    sx, sy = rng.uniform(60, W - 60, nspots), rng.uniform(60, H - 60, nspots)
    base = rng.integers(0, 256, (nspots, 32), dtype=np.uint8)

    def near(d, n):
        u = np.unpackbits(d.copy())
        u[rng.choice(256, n, replace=False)] ^= 1
        return np.packbits(u)
    x2 = np.repeat(sx, per2) + rng.uniform(-6, 6, nspots * per2)
    y2 = np.repeat(sy, per2) + rng.uniform(-6, 6, nspots * per2)
    d2 = np.stack([near(base[s], 3 * k) for s in range(nspots) for k in rng.permutation(per2)])
    x1 = np.repeat(sx, per1) + rng.uniform(-6, 6, nspots * per1)
    y1 = np.repeat(sy, per1) + rng.uniform(-6, 6, nspots * per1)
    d1 = np.stack([near(base[s], int(rng.integers(0, 2))) for s in range(nspots) for _ in range(per1)])
    t1 = table(x1, y1, d1, angle=wrap360(rng.uniform(0, 360, len(x1))))
    t2 = table(x2, y2, d2, angle=wrap360(rng.uniform(0, 360, len(x2))))
    return t1, t2


def test_windows_with_more_candidates_than_the_list(fe):
    t1, t2 = crowded(np.random.default_rng(8))
    lists = init_candidates(t1, t2, points_of(t1), BOUNDS, 20, dist_limit(0.9))
    sizes = [len(l[0]) for l in lists]
    assert min(sizes) > LIST_WIDTH, min(sizes)                                # every window overflows the list
    for check_ori in (False, True):
        nm, m12, raw, _ = check(fe, t1, t2, window=20, check_ori=check_ori, scalar=not check_ori)
        assert int((raw >= 0).sum()) > 20
    t1m, t2m = crowded(np.random.default_rng(9), per2=LIST_WIDTH)              # exactly the width, and mixed with wider ones
    t2x = table(np.concatenate([t2m.x, t2.x]), np.concatenate([t2m.y, t2.y]), np.concatenate([t2m.desc, t2.desc]),
                angle=np.concatenate([t2m.angle, t2.angle]))
    t1x = table(np.concatenate([t1m.x, t1.x]), np.concatenate([t1m.y, t1.y]), np.concatenate([t1m.desc, t1.desc]),
                angle=np.concatenate([t1m.angle, t1.angle]))
    nm, _, _, _ = check(fe, t1x, t2x, window=20)
    assert nm > 20


def test_real_orb_tables(fe):
    """Tables of the device's own extractor (as real_case of tests/test_fuse_search_gpu.py gets them): the left image of frame 0
    against its right image, the next frame and itself, chained, window 100."""
    total = 0
    frames = realdata.frames_752x480(2, seed=4)
    for pair in ([synth.make_stereo_pair(3, W, H, t=0), synth.make_stereo_pair(3, W, H, t=1)], [frames[0], frames[1]]):
        rec0, rec1 = stereo_frame(fe, *pair[0]), stereo_frame(fe, *pair[1])

        def tab(kp, desc):
            return table(kp["x"], kp["y"], desc.copy(), kp["octave"], kp["angle"])
        t1 = tab(rec0["kpL"], rec0["descL"])
        prev = points_of(t1)
        for t2 in (tab(rec0["kpR"], rec0["descR"]), tab(rec1["kpL"], rec1["descL"]), t1):
            nm, _, _, prev = check(fe, t1, t2, prev, window=100)
            total += nm
    print("real ORB tables: %d matches" % total)
    assert total > 200, total                 # a table against itself alone matches its octave-0 keypoints with a unique descriptor


def random_table(rng, n, octave0=0.6):
    return table(rng.uniform(0, W, n), rng.uniform(0, H, n), rng.integers(0, 256, (n, 32), dtype=np.uint8),
                 (rng.random(n) > octave0).astype(np.int32) * rng.integers(1, NLEVELS, n), wrap360(rng.uniform(0, 360, n)))


def test_the_cap_and_one_above(fe):
    rng = np.random.default_rng(5)
    full1, full2, small = random_table(rng, CAP), random_table(rng, CAP), random_table(rng, 60)
    # copies of F1 rows in F2, so that matches happen at the cap: the last rows too
    pick = np.concatenate([rng.choice(CAP, 600, replace=False), [CAP - 1]])
    full2.desc[pick] = full1.desc[pick]
    full2.x[pick], full2.y[pick], full2.octave[pick] = full1.x[pick] + 3, full1.y[pick], 0
    full1.octave[pick] = 0
    nm, _, raw, _ = check(fe, full1, full2, window=12)                         # n1 and n2 exactly at the cap
    assert int((raw >= 0).sum()) > 300 and nm > 100 and raw[CAP - 1] == CAP - 1
    big = random_table(rng, CAP + 1)
    for a, b in ((big, small), (small, big)):
        with pytest.raises(capi.PliError) as e:
            call(fe, a, b)
        assert e.value.status == -3                                           # PLI_ERR_CAPACITY


def test_errors_null_pointers_and_empty_sides(fe):
    rng = np.random.default_rng(3)
    t1, t2 = random_table(rng, 50), random_table(rng, 70)
    for kw in (dict(window=-1), dict(nnratio=0.0), dict(nnratio=-0.5), dict(nnratio=float("nan")), dict(nnratio=float("inf"))):
        with pytest.raises(capi.PliError) as e:
            call(fe, t1, t2, **kw)
        assert e.value.status == -1, kw                                       # PLI_ERR_INVALID
    for side in (0, 1):
        for octave in (-1, NLEVELS):
            bad = [t1, t2]
            bad[side] = bad[side]._replace(octave=np.concatenate([bad[side].octave[:-1], [octave]]).astype(np.int32))
            with pytest.raises(capi.PliError) as e:
                call(fe, *bad)
            assert e.value.status == -1
        for angle in (360.0, -1.0, float("nan")):
            bad = [t1, t2]
            bad[side] = bad[side]._replace(angle=np.concatenate([bad[side].angle[:-1], [angle]]).astype(np.float32))
            with pytest.raises(capi.PliError) as e:
                call(fe, *bad)
            assert e.value.status == -1
            check(fe, *bad, check_ori=False)                                  # the angles are not read without it
    prev = points_of(t1)
    prev[17, 1] = np.nan
    with pytest.raises(capi.PliError) as e:
        call(fe, t1, t2, prev)
    assert e.value.status == -1
    check(fe, t1, t2, nnratio=1e-3)
    # empty sides
    empty = table([], [], np.zeros((0, 32), np.uint8))
    for a, b in ((empty, t2), (t1, empty), (empty, empty)):
        nm, m12, raw, p = check(fe, a, b)
        assert nm == 0 and len(m12) == len(a.x) and (m12 == -1).all() and (raw == -1).all()
    # raw calls: every null pointer
    L, h, ptr = fe.L, fe.h, capi.ptr
    k1, k2, d1, d2 = keypoints(t1), keypoints(t2), np.ascontiguousarray(t1.desc), np.ascontiguousarray(t2.desc)
    pm = points_of(t1)
    m12, raw = np.zeros(50, np.int32), np.zeros(50, np.int32)
    nmo = C.c_int32()

    def rawcall(h=h, k1=k1, d1=d1, pm=pm, k2=k2, d2=d2, m=m12, r=raw, nm=nmo, n1=50, n2=70):
        return L.pli_search_for_initialization(h, ptr(k1), ptr(d1), n1, ptr(pm), ptr(k2), ptr(d2), n2, 0.0, 752.0, 0.0, 480.0, 100, 0.9,
                                               1, ptr(m), ptr(r), C.byref(nm) if nm is not None else None)
    assert rawcall() == 0
    assert rawcall(r=None) == 0                                               # raw12 may be NULL
    for kw in (dict(h=None), dict(k1=None), dict(d1=None), dict(pm=None), dict(k2=None), dict(d2=None), dict(m=None), dict(nm=None)):
        assert rawcall(**kw) == -1, kw
    assert rawcall(n1=-1) == -1 and rawcall(n2=-1) == -1
    assert L.pli_search_for_initialization(h, ptr(k1), ptr(d1), 50, ptr(pm), ptr(k2), ptr(d2), 70, 0.0, 0.0, 0.0, 480.0, 100, 0.9, 1,
                                           ptr(m12), ptr(raw), C.byref(nmo)) == -1      # empty image bounds


def test_a_repeated_call_gives_identical_output(fe):
    t1, (t2, t3, _) = scene(np.random.default_rng(SCENE_SEED + 2))
    first = call(fe, t1, t2)
    other = call(fe, t1, t3)                                                  # another call in between reuses the scratch
    for _ in range(2):
        again = call(fe, t1, t2)
        assert again[0] == first[0] and all(np.array_equal(a, b) for a, b in zip(again[1:], first[1:]))
    assert not np.array_equal(other[1], first[1])
