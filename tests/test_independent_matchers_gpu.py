"""The stereo kernels on constructed tables, and the descriptor matchers, against tests/helpers_matchers.py (and therefore
against the oracle, see test_independent_matchers.py): the same corpus through the C ABI, every output bit-equal.

k_stereo_points, k_stereo_median and k_stereo_lines read their tables from the result record, so constructed tables need no
entry point of their own (the route is described next to Frontend.batch_run_device): run the whole front-end on the case's
images, overwrite counts / keypoints / descriptors / keylines / line descriptors of the record on the device, run the two
stereo stages alone, read uright, depth, disp, le, counts[4], counts[5] and, through DBG_STEREO_SAD, the SADs and best indices.

Every table passes helpers_matchers.validate_tables with the context's capacities before it goes to the device.
"""
import numpy as np
import pytest

import helpers_matchers as hm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def po():
    from oracle import pyoracle
    pyoracle.lib()
    return pyoracle


corpus, run_points = hm.stereo_corpus, hm.run_points


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from pli_slam_amd import capi
    from pli_slam_amd.frontend import Frontend

    class G:
        pass
    g = G()
    g.capi, g.Frontend, g.torch = capi, Frontend, torch
    return g


def group_key(c):
    return bytes(c["cfg"])


def run_batch(g, fe, cases):
    """cases: one per frame of the batch.  -> per frame (record dict, sad, best_idx)."""
    torch, capi = g.torch, g.capi
    Y = fe.layout
    F = len(cases)
    W, H = fe.cfg.width, fe.cfg.height
    imgs = np.full((F, 2, H, W), 100, np.uint8)
    for f, c in enumerate(cases):
        hm.validate_tables(c, kp_cap=fe.kp_cap, kl_cap=fe.kl_cap)
        assert (c["W"], c["H"], c["nlevels"]) == (W, H, fe.cfg.orb_nlevels)
        if c["L"] is not None:
            imgs[f, 0], imgs[f, 1] = c["L"], c["R"]
    dimg = torch.from_numpy(imgs).cuda()
    dtab = torch.zeros(fe.table_bytes(F), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    args = (F, dimg.data_ptr(), dimg.data_ptr() + W * H, W, 2 * W * H, dtab.data_ptr())
    fe.batch_run_device(*args, stages=capi.RUN_ALL)
    fe.sync()
    tab = dtab.cpu().numpy().copy()
    for f, c in enumerate(cases):
        rec = tab[f * Y.record_bytes:(f + 1) * Y.record_bytes]
        counts = rec[Y.off_counts:Y.off_counts + 32].view(np.int32)
        counts[0], counts[1], counts[2], counts[3] = len(c["kpL"]), len(c["kpR"]), len(c["klL"]), len(c["klR"])
        counts[4] = counts[5] = -7                      # (must be rewritten by the stereo stages)
        for e, k in enumerate("LR"):
            for off, arr in ((Y.off_kp[e], c["kp" + k]), (Y.off_desc[e], c["desc" + k]), (Y.off_kl[e], c["kl" + k]),
                             (Y.off_ldesc[e], c["ld" + k])):
                b = np.ascontiguousarray(arr).view(np.uint8).ravel()
                rec[off:off + b.size] = b
        n, m = len(c["kpL"]), len(c["klL"])
        rec[Y.off_uright:Y.off_uright + 4 * n].view(np.float32)[:] = 123.0
        rec[Y.off_depth:Y.off_depth + 4 * n].view(np.float32)[:] = 123.0
        rec[Y.off_disp:Y.off_disp + 8 * m].view(np.float32)[:] = 123.0
        rec[Y.off_le:Y.off_le + 24 * m].view(np.float64)[:] = 123.0
    dtab.copy_(torch.from_numpy(tab))
    torch.cuda.synchronize()
    fe.batch_run_device(*args, stages=capi.RUN_STEREO_POINTS | capi.RUN_STEREO_LINES)
    fe.sync()
    tab = dtab.cpu().numpy()
    out = []
    for f in range(F):
        raw = fe.debug_fetch(2 * f, capi.DBG_STEREO_SAD).view(np.int32)
        out.append((fe.parse_record(tab, f), raw[:fe.kp_cap].copy(), raw[fe.kp_cap:2 * fe.kp_cap].copy()))
    return out


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


def make_frontend(g, c, max_frames, lsd_nfeatures):
    cfg = g.capi.Config.from_buffer_copy(bytes(c["cfg"]))
    cfg.max_frames, cfg.orb_nfeatures, cfg.lsd_nfeatures = max_frames, 2000, lsd_nfeatures
    fe = g.Frontend(cfg)
    fe.debug_enable(True)
    return fe


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
