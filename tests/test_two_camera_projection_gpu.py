"""pli_search_by_projection_two_cameras on the MI355X (the product library): ORBmatcher::SearchByProjection(CurrentFrame, LastFrame,
th, bMono) for a current frame of two cameras (ORBmatcher.cc:1961-2177) equals the line-by-line restatement of
tests/test_two_camera_projection_cpu.py exactly (nmatches, best_left / best_right, raw_left / raw_right).  That file shows, on the
CPU, that the constructed scene takes every exit of the two-camera branch, so the equalities here are not vacuous."""
import ctypes as C

import numpy as np
import pytest

from pli_slam_amd import capi
from test_two_camera_projection_cpu import (CAPACITY_CASES, GRID_INSIDE_BOUNDS, INVALID_VALID_VALUES, PLI_ERR_INVALID, PLI_OK,
                                            constructed_scene, expected, hand_worked_cases, random_tables)

pytestmark = pytest.mark.gpu
W, H = 752, 480


@pytest.fixture(scope="module")
def fe():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from pli_slam_amd.frontend import Frontend
    f = Frontend(capi.default_config(W, H), dev=False)
    yield f
    f.close()


def call(fe, T, check_ori=True, with_occ=True, with_raw=True):
    occ = dict(occ_left=T["occ_left"], occ_right=T["occ_right"]) if with_occ else {}
    return fe.search_by_projection_two_cameras(T["q_left"], T["q_right"], T["qdesc"], T["kp_left"], T["desc_left"], T["kp_right"],
                                               T["desc_right"], T["bounds"], check_ori, with_raw=with_raw, **occ)


def check(fe, name, make, check_ori=True, with_occ=True):
    T, want = expected(name, make, check_ori, with_occ)
    got = call(fe, T, check_ori, with_occ)
    for what, g, w in zip(("best_left", "best_right", "raw_left", "raw_right"), got[1:], want[1:5]):
        assert np.array_equal(g, w), "%s: %d of %d %s differ" % (name, int((g != w).sum()), len(w), what)
    assert got[0] == want[0], (name, got[0], want[0])
    return got


@pytest.mark.parametrize("check_ori", [True, False])
def test_constructed_scene(fe, check_ori):
    n, bl, br, rl, rr = check(fe, "scene", lambda: constructed_scene()[0], check_ori)
    accepts = int((rl >= 0).sum() + (rr >= 0).sum())
    print("check_orientation %d: %d accepts, %d returned" % (check_ori, accepts, n))
    assert accepts == 57 and n == (45 if check_ori else 57)                  # the figures of the CPU file's docstring
    check(fe, "scene", lambda: constructed_scene()[0], check_ori, with_occ=False)
    # without raw_*: the same best_* and count
    T, want = expected("scene", lambda: constructed_scene()[0], check_ori)
    got = call(fe, T, check_ori, with_raw=False)
    assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])


def test_hand_worked_cases(fe):
    for name, T, check_ori, n, bl, br, rl, rr in hand_worked_cases():
        got = check(fe, "hand_" + name, T, check_ori)
        assert got[0] == n and [g.tolist() for g in got[1:]] == [bl, br, rl, rr], name


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_tables(fe, seed):
    check(fe, "random_%d" % seed, lambda: random_tables(seed))               # nq = 400, nleft = 350, nright = 300
    if seed == 1:
        check(fe, "random_1", lambda: random_tables(1), True, with_occ=False)


def test_dense_windows_straddle_the_candidate_list(fe):
    check(fe, "dense", lambda: random_tables(5, nq=60, nl=300, nr=260, dense=True))


def test_bounds_that_leave_keypoints_outside_the_grid(fe):
    check(fe, "inside", lambda: random_tables(6, bounds=GRID_INSIDE_BOUNDS))


def test_no_right_camera_equals_the_one_camera_search(fe):
    """nright == 0 and every row valid: the existing pli_search_by_projection on the left table with no right coordinates (device
    against device)."""
    T = random_tables(8, nq=300, nl=320, nr=0)
    T["q_left"]["valid"] = np.where(T["q_left"]["valid"] == 0, 1, T["q_left"]["valid"])
    n, bl, br, rl, rr = call(fe, T)
    n1, best, raw = fe.search_by_projection(T["q_left"], T["qdesc"], T["kp_left"], T["desc_left"], np.full(320, -1, np.float32), T["bounds"],
                                            True, T["occ_left"], with_raw=True)
    assert n == n1 > 10 and np.array_equal(bl, best) and np.array_equal(rl, raw)
    assert (br == -1).all() and (rr == -1).all()


def test_empty_tables(fe):
    T = random_tables(9, nq=200, nl=0, nr=250)                              # no left keypoint: every left window is empty
    n, bl, br, rl, rr = check(fe, "no_left", T)
    assert n == 0 and (br == -1).all()
    T = random_tables(9, nq=0, nl=50, nr=40)
    n, bl, br, rl, rr = call(fe, T)
    assert n == 0 and len(bl) == len(br) == len(rl) == len(rr) == 0
    T = random_tables(9, nq=20, nl=0, nr=0)
    assert call(fe, T)[0] == 0


def _raw_call(fe, T, nl=None, nr=None):
    L, ptr = fe.L, capi.ptr
    nq = len(T["q_left"])
    out = [np.full(nq, -7, np.int32) for _ in range(4)]
    n = C.c_int32(-7)
    st = L.pli_search_by_projection_two_cameras(fe.h, ptr(T["q_left"]), ptr(T["q_right"]), ptr(T["qdesc"]), nq, ptr(T["kp_left"]),
                                                ptr(T["desc_left"]), None, len(T["kp_left"]) if nl is None else nl, ptr(T["kp_right"]),
                                                ptr(T["desc_right"]), None, len(T["kp_right"]) if nr is None else nr, *T["bounds"], 1,
                                                ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3]), C.byref(n))
    return st, n.value, out


@pytest.mark.parametrize("nl,nr,status", CAPACITY_CASES)
def test_the_lds_capacity(fe, nl, nr, status):
    """nleft + nright == 15360 runs (the larger owner table fills its block's LDS share) and equals the restatement; one more is
    PLI_ERR_CAPACITY with nothing written."""
    T = random_tables(10, nq=6, nl=nl, nr=nr)
    st, n, out = _raw_call(fe, T)
    assert st == status
    if status == PLI_OK:
        _, want = expected("capacity_%d_%d" % (nl, nr), T, True, False)
        assert n == want[0] and all(np.array_equal(g, w) for g, w in zip(out, want[1:5]))
    else:
        assert n == 0 and all((o == -7).all() for o in out)


@pytest.mark.parametrize("valid", INVALID_VALID_VALUES)
def test_unknown_valid_bits_are_refused(fe, valid):
    T = random_tables(11, nq=30, nl=40, nr=40)
    T["q_left"]["valid"][17] = valid
    st, n, out = _raw_call(fe, T)
    assert st == PLI_ERR_INVALID and n == 0 and all((o == -7).all() for o in out)
    T["q_left"]["valid"][17] = 1
    T["q_right"]["valid"][:] = valid                                         # q_right.valid is not read
    assert _raw_call(fe, T)[0] == PLI_OK


def test_two_consecutive_calls_return_the_same_bytes(fe):
    T, _ = expected("random_2", lambda: random_tables(2))
    a = call(fe, T)
    b = call(fe, T)
    assert a[0] == b[0] and all(x.tobytes() == y.tobytes() for x, y in zip(a[1:], b[1:]))
