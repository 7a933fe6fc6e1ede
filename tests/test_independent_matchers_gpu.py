"""The stereo kernels on constructed tables, and the descriptor matchers, against tests/helpers_matchers.py (and therefore
against the oracle, see test_independent_matchers.py): the same corpus through the C ABI, every output bit-equal.

The route that puts constructed tables in front of the stereo kernels is tests/helpers_stereo_gpu.py: run_batch.
"""
import numpy as np
import pytest

import helpers_matchers as hm
from helpers_stereo_gpu import device, group_key, make_frontend, run_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def po():
    from oracle import pyoracle
    pyoracle.lib()
    return pyoracle


corpus, run_points = hm.stereo_corpus, hm.run_points


@pytest.fixture(scope="module")
def gpu():
    return device()


def check(c, got, po_):
    rec, sad, bidx = got
    n = len(c["kpL"])
    if c["pyr"] is not None:
        ur, dp, bi, sd, _, _ = run_points(c)
        for name, a, b in (("uright", rec["uright"], ur), ("depth", rec["depth"], dp), ("best_idx", bidx[:n], bi), ("sad", sad[:n], sd)):
            bad = np.flatnonzero(a.view(np.int32) != b.view(np.int32))
            assert bad.size == 0, "%s: %s differs at left keypoints %s" % (c["name"], name, bad[:5])
        assert rec["counts"][4] == int((ur >= 0).sum()), c["name"]
    disp, le, _, _ = hm.stereo_lines(c["cfg"], c["klL"], c["ldL"], c["klR"], c["ldR"], c["W"], c["H"])
    assert rec["disp"].tobytes() == disp.tobytes(), "%s: disp differs at %s" % (c["name"], np.flatnonzero((rec["disp"] != disp).any(1))[:5])
    assert rec["le"].tobytes() == le.tobytes(), "%s: le" % c["name"]
    assert rec["counts"][5] == int((disp[:, 0] >= 0).sum()), c["name"]


@pytest.mark.parametrize("lsd_nfeatures,sliced", [(160, False), (256, True)])
def test_stereo_kernels_on_the_corpus(gpu, po, lsd_nfeatures, sliced):
    """One frame per call and four frames per call with different tables per frame (the kernels index scratch by frame);
    kl_cap < 192: the line matcher in one launch (phase 0); kl_cap >= 192: the sliced phases 1-3, on the same tables."""
    g = gpu
    groups = {}
    for c in corpus(po):
        groups.setdefault(group_key(c), []).append(c)
    ncase = 0
    for key, cases in groups.items():
        fe = make_frontend(g, cases[0], 4, lsd_nfeatures)
        assert (fe.kl_cap >= 192) == sliced, fe.kl_cap
        for i in range(0, len(cases), 4):
            chunk = cases[i:i + 4]
            for c, got in zip(chunk, run_batch(g, fe, chunk)):
                check(c, got, po)
                ncase += 1
        # one frame per call; and the same tables in another frame slot than before
        check(cases[-1], run_batch(g, fe, [cases[-1]])[0], po)
        if len(cases) > 1:
            rev = cases[:4][::-1]
            for c, got in zip(rev, run_batch(g, fe, rev)):
                check(c, got, po)
        fe.close()
    assert ncase == len(corpus(po))


def test_descriptor_matchers_on_the_shared_tables(gpu):
    g = gpu
    fe = g.Frontend(g.capi.default_config(128, 128))
    a, b, c, d = hm.descriptor_tables_random_and_ties()
    idx, dist = fe.knn2(a, b)
    ridx, rdist = hm.knn2(a, b)
    assert np.array_equal(idx, ridx) and np.array_equal(dist, rdist)
    for q, t in ((a, b), (c, d), (a[:5], b[:2])):
        for nnr in (0.9, 0.75, 1.0):
            n, m = fe.match_nnr(q, t, nnr)
            rn, rm = hm.match_nnr(q, t, nnr)
            assert n == rn and np.array_equal(m, rm)
            n, m = fe.match(q, t, nnr)
            rn, rm = hm.match_lines(q, t, nnr, True)
            assert n == rn and np.array_equal(m, rm)
    for q, t, d0, d1 in hm.nnr_float_boundary_tables():
        for nnr in (0.9, 0.6):
            n, m = fe.match_nnr(q, t, nnr)
            rn, rm = hm.match_nnr(q, t, nnr)
            assert n == rn and np.array_equal(m, rm), (d0, d1, nnr)


def test_projection_searches_on_the_constructed_cases(gpu):
    g = gpu
    fe = g.Frontend(g.capi.default_config(128, 128))
    for c in hm.build_projection_cases():
        for occ in (None, c["occ"]):
            for ori in (True, False):
                n, best, raw = fe.search_by_projection(c["q"], c["qd"], c["kp"], c["desc"], c["ur"], c["bounds"], ori, occupied=occ, with_raw=True)
                rn, rbest, rraw, _, _ = hm.search_by_projection(c["q"], c["qd"], c["kp"], c["desc"], c["ur"], c["bounds"], ori, occ)
                assert n == rn and np.array_equal(best, rbest) and np.array_equal(raw, rraw), (c["name"], occ is not None, ori)
            for nnratio in (0.8, 0.5, 1.0):
                n, best = fe.search_local_map(c["q"], c["qd"], c["kp"], c["desc"], c["ur"], c["bounds"], nnratio, cur_occupied=occ)
                rn, rbest, _ = hm.search_local_map(c["q"], c["qd"], c["kp"], c["desc"], c["ur"], occ, c["bounds"], nnratio)
                assert n == rn and np.array_equal(best, rbest), (c["name"], occ is not None, nnratio)


def test_projection_searches_on_the_random_generators(gpu):
    g = gpu
    fe = g.Frontend(g.capi.default_config(128, 128))
    q, qd, kp, desc, ur, bounds = hm.local_map_ties_tables()
    for nnratio in (0.8, 0.5, 1.0):
        n, best = fe.search_local_map(q, qd, kp, desc, ur, bounds, nnratio)
        rn, rbest, _ = hm.search_local_map(q, qd, kp, desc, ur, None, bounds, nnratio)
        assert n == rn and np.array_equal(best, rbest)
    q, qd, kp, desc, ur, occ, bounds, rng = hm.dense_window_tables(3000, 1500)
    n, best = fe.search_local_map(q, qd, kp, desc, ur, bounds, 0.8, cur_occupied=occ)
    rn, rbest, _ = hm.search_local_map(q, qd, kp, desc, ur, occ, bounds, 0.8)
    assert n == rn and np.array_equal(best, rbest)
    qn = q.copy()
    qn["valid"] = np.where((qn["valid"] != 0) & (rng.random(len(q)) < 0.4), 3, qn["valid"])
    for ori in (True, False):
        n, best, raw = fe.search_by_projection(qn, qd, kp, desc, ur, bounds, ori, occupied=occ, with_raw=True)
        rn, rbest, rraw, _, _ = hm.search_by_projection(qn, qd, kp, desc, ur, bounds, ori, occ)
        assert n == rn and np.array_equal(best, rbest) and np.array_equal(raw, rraw)
