"""Known-answer tests of the oracle (CPU restatement of the reference path).

The reference ships no tests or golden vectors for this path, so these
are the build's own KATs: each checks the oracle against a value derived
by hand or by an independent formula, not against the HIP code.
"""
import numpy as np
import pytest

from pli_slam_amd import synth


def test_descriptor_distance_kats(oracle):
    z = np.zeros((1, 32), np.uint8)
    o = np.full((1, 32), 255, np.uint8)
    assert oracle.descriptor_distance(z, o)[0] == 256
    assert oracle.descriptor_distance(z, z)[0] == 0
    one = z.copy(); one[0, 17] = 0x10
    assert oracle.descriptor_distance(z, one)[0] == 1
    rng = np.random.default_rng(1)
    a = rng.integers(0, 256, (500, 32), dtype=np.uint8)
    b = rng.integers(0, 256, (500, 32), dtype=np.uint8)
    want = np.unpackbits(a ^ b, axis=1).sum(1)
    assert np.array_equal(oracle.descriptor_distance(a, b), want)


def test_cv_round_half_even(oracle):
    assert [oracle.cv_round(v) for v in (0.5, 1.5, 2.5, -0.5, -1.5, 2.4999, 2.5001)] == [0, 2, 2, 0, -2, 2, 3]


def test_fast_atan2(oracle):
    # exact axes and quadrants; polynomial error bound of cv::fastAtan2 is ~0.3 degrees
    assert oracle.fast_atan2(0.0, 1.0) == 0.0
    assert abs(oracle.fast_atan2(1.0, 0.0) - 90.0) < 1e-4
    assert abs(oracle.fast_atan2(0.0, -1.0) - 180.0) < 1e-4
    assert abs(oracle.fast_atan2(-1.0, 0.0) - 270.0) < 1e-4
    rng = np.random.default_rng(2)
    for y, x in rng.normal(size=(200, 2)):
        want = np.degrees(np.arctan2(y, x)) % 360.0
        got = oracle.fast_atan2(float(y), float(x))
        assert abs((got - want + 180) % 360 - 180) < 0.3


def test_gauss_kernels(oracle):
    # 8-bit fixed point kernels of the three blurs on the path
    assert oracle.gauss_kernel(7, 2.0).tolist() == [18, 34, 49, 55, 49, 34, 18]       # ORB, ORBextractor.cc:1115
    assert oracle.gauss_kernel(5, 1.0).tolist() == [14, 63, 103, 63, 14]              # LBD, binary_descriptor_custom.cpp:358
    assert oracle.gauss_kernel(7, 0.6).tolist() == [0, 1, 42, 170, 42, 1, 0]          # LSD pre-filter


def test_blur_constant_image_is_fixed_point_gain(oracle):
    img = np.full((40, 50), 100, np.uint8)
    # sum of the 7x7 sigma-2 integer kernel is 257: (100*257*257 + 2^15) >> 16 = 101
    assert np.all(oracle.gaussian_blur(img, 7, 2.0) == 101)
    assert np.all(oracle.gaussian_blur(img, 5, 1.0) == 101)                          # 5x5 sigma-1 kernel sums to 257 too
    assert np.all(oracle.gaussian_blur(img, 7, 0.6) == 100)                          # LSD pre-filter kernel sums to 256


def test_resize_identity_and_downscale(oracle):
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (48, 60), dtype=np.uint8)
    assert np.array_equal(oracle.resize(img, 60, 48, 1.0, 1.0), img)
    flat = np.full((48, 60), 77, np.uint8)
    assert np.all(oracle.resize(flat, 50, 40, 60 / 50, 48 / 40) == 77)
    assert np.all(oracle.resize(flat, 72, 58, 1 / 1.2, 1 / 1.2) == 77)


def test_sobel_ramp(oracle):
    x = np.tile(np.arange(30, dtype=np.uint8) * 3, (20, 1))
    dx, dy = oracle.sobel(x)
    assert np.all(dx[:, 1:-1] == 24) and np.all(dy == 0)     # (1+2+1) * 2*3
    assert np.all(dx[:, 0] == 0) and np.all(dx[:, -1] == 0)  # REFLECT_101 makes the border derivative vanish


def test_fast_arc_values(oracle):
    img = np.full((15, 15), 100, np.uint8)
    assert oracle.fast_arc(img, 7, 7) == 0                    # flat: not a corner at any threshold
    img[7, 7] = 160                                           # bright dot: every ring pixel is darker by 60
    assert oracle.fast_arc(img, 7, 7) == 60
    img2 = np.full((15, 15), 100, np.uint8)
    ring = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3)]
    for k, (dx, dy) in enumerate(ring):
        img2[7 + dy, 7 + dx] = 130 + k                        # 9 contiguous brighter pixels, weakest is +30
    assert oracle.fast_arc(img2, 7, 7) == 30
    img2[7 + 3, 7 + 0] = 100                                  # break the arc: 8 contiguous only
    assert oracle.fast_arc(img2, 7, 7) < 1


def test_brief_constant_image_is_zero(oracle):
    img = np.full((64, 64), 90, np.uint8)
    for ang in (0.0, 37.5, 90.0, 271.0):
        assert not oracle.orb_descriptor(img, 32, 32, ang).any()


def test_brief_rotation_consistency(oracle):
    # rotating the image by 90 degrees and the keypoint angle by 90 degrees gives the same bits
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (65, 65), dtype=np.uint8)
    d0 = oracle.orb_descriptor(img, 32, 32, 0.0)
    rot = np.ascontiguousarray(np.rot90(img, -1))             # 90 degrees clockwise in image coordinates (y down)
    d90 = oracle.orb_descriptor(rot, 32, 32, 90.0)
    assert np.array_equal(d0, d90)


def test_features_per_level_and_umax(oracle):
    f = oracle.Frame(oracle.default_config(752, 480))
    assert f.features_per_level().tolist() == [261, 217, 181, 151, 126, 105, 87, 72]
    assert f.umax().tolist() == [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]


def test_orb_blank_and_empty_images(oracle):
    f = oracle.Frame(oracle.default_config(320, 240))
    n, kp, desc = f.orb_extract(0, np.full((240, 320), 128, np.uint8))
    assert n == 0
    n, _, _ = f.orb_extract(0, None)
    assert n == -1                                             # ORBextractor.cc:1072


def test_orb_pipeline_invariants(oracle):
    L, _ = synth.make_stereo_pair(4, 320, 240)
    cfg = oracle.default_config(320, 240, orb_nfeatures=400)
    f = oracle.Frame(cfg)
    n, kp, desc = f.orb_extract(0, L)
    assert 0 < n <= 400 + 3 * 8
    assert np.all(np.diff(kp["octave"]) >= 0)                  # level-major output order
    quota = f.features_per_level()
    scale = np.float32(1.0)
    for l in range(8):
        sel = f.level_points(0, l, selected=True)
        cand = f.level_points(0, l)
        assert len(sel) <= max(quota[l] + 3, 8)
        assert set(map(tuple, sel.tolist())) <= set(map(tuple, cand.tolist()))
        im = f.pyramid(0, l)
        k = kp[kp["octave"] == l]
        xs = np.rint(k["x"] / scale).astype(int); ys = np.rint(k["y"] / scale).astype(int)
        assert np.all((xs >= 19) & (xs < im.shape[1] - 19) & (ys >= 19) & (ys < im.shape[0] - 19))
        scale = np.float32(scale * np.float32(1.2))
    # the extractor is a pure function of the image
    n2, kp2, desc2 = oracle.Frame(cfg).orb_extract(0, L)
    assert n2 == n and kp2.tobytes() == kp.tobytes() and np.array_equal(desc, desc2)


def test_lsd_rectangle(oracle):
    img = np.full((240, 320), 40, np.uint8)
    img[60:180, 80:240] = 200
    cfg = oracle.default_config(320, 240, lsd_nfeatures=0)
    f = oracle.Frame(cfg)
    n, kl, desc = f.line_extract(0, img)
    segs = f.lsd_segments(0)
    want = [((80, 60), (240, 60)), ((80, 180), (240, 180)), ((80, 60), (80, 180)), ((240, 60), (240, 180))]
    for (a, b) in want:
        best = 1e9
        for s in segs:
            for p, q in (((s[0], s[1]), (s[2], s[3])), ((s[2], s[3]), (s[0], s[1]))):
                # distance of both detected endpoints to the ideal edge line, and coverage of its length
                def dline(pt):
                    (x1, y1), (x2, y2) = a, b
                    return abs((x2 - x1) * (y1 - pt[1]) - (x1 - pt[0]) * (y2 - y1)) / np.hypot(x2 - x1, y2 - y1)
                cover = np.hypot(p[0] - q[0], p[1] - q[1]) / np.hypot(a[0] - b[0], a[1] - b[1])
                if cover > 0.9:
                    best = min(best, max(dline(p), dline(q)))
        assert best < 1.0, (a, b, best)                        # edges sit between pixel rows: < 1 px off the ideal line
    assert n >= 4 and desc.shape == (n, 32)
    assert np.all(kl["numOfPixels"] >= 1) and np.all(kl["lineLength"] > 0.025 * 240)


def test_line_topn_is_stable_by_response(oracle):
    L, _ = synth.make_stereo_pair(2, 320, 240)
    allc = oracle.default_config(320, 240, lsd_nfeatures=0)
    topc = oracle.default_config(320, 240, lsd_nfeatures=20)
    fa, ft = oracle.Frame(allc), oracle.Frame(topc)
    na, kla, _ = fa.line_extract(0, L)
    nt, klt, _ = ft.line_extract(0, L)
    assert nt == 20 and na > 20
    order = np.argsort(-kla["response"], kind="stable")[:20]
    assert np.array_equal(klt["startPointX"], kla["startPointX"][order])
    assert klt["class_id"].tolist() == list(range(20))


def test_lbd_weights(oracle):
    Lw, G = oracle.lbd_weights()
    # integer-division quirk of the reference: u = 10, sigma = 7 (local); u = sigma = 31 (global)
    assert np.allclose(Lw, np.exp(-((np.arange(21) - 10.0) ** 2) / (2 * 49.0)).astype(np.float32))
    assert np.allclose(G, np.exp(-((np.arange(63) - 31.0) ** 2) / (2 * 961.0)).astype(np.float32))


def test_stereo_integer_shift(oracle):
    # right image = left shifted by d px: uRight = uL - d for every matched keypoint
    d = 12
    big, _ = synth.make_stereo_pair(6, 320 + d, 240)
    left = np.ascontiguousarray(big[:, :320])
    right = np.ascontiguousarray(big[:, d:320 + d])           # a point at uL appears at uL - d
    f = oracle.Frame(oracle.default_config(320, 240, orb_nfeatures=500))
    nl, kp, _ = f.orb_extract(0, left)
    f.orb_extract(1, right)
    ur, depth, bi, sad = f.stereo_points()
    m = ur >= 0
    assert m.sum() > 0.3 * nl
    err = np.abs((kp["x"][m] - ur[m]) - d)
    scale = np.float32(1.2) ** kp["octave"][m]
    assert np.all(err <= 0.6 * scale)                          # coordinates are rounded at the keypoint's pyramid level
    assert np.median(err) < 0.25
    assert np.allclose(depth[m], np.float32(oracle.default_config(320, 240).bf) / (kp["x"][m] - ur[m]), rtol=1e-6)


def test_match_and_knn_small_cases(oracle):
    a = np.zeros((3, 32), np.uint8)
    b = np.zeros((4, 32), np.uint8)
    a[0, 0] = 0b1; a[1, 0] = 0b11; a[2, :] = 255
    b[0, 0] = 0b1; b[1, 0] = 0b111; b[2, :] = 255; b[3, :16] = 255
    idx, dist = oracle.knn2(a, b)
    assert idx[0].tolist() == [0, 1] and dist[0].tolist() == [0, 2]
    assert idx[1].tolist() == [0, 1] and dist[1].tolist() == [1, 1]      # tie -> lower train index first
    assert idx[2].tolist() == [2, 3] and dist[2].tolist() == [0, 128]
    n, m = oracle.match_lines(a, b, 0.9, True)
    assert m.tolist() == [0, -1, 2] and n == 2                           # a[1]: 1 < 0.9*1 fails


def test_match_grid_prefix_min_rule(oracle):
    # two left lines see the same right line; the second has the smaller distance.  With bestLRMatches
    # the first is accepted by the ratio test but loses the mutual check (LineMatcher.cpp:360-393).
    kl = np.zeros(2, oracle.KEYLINE_DT)
    kr = np.zeros(1, oracle.KEYLINE_DT)
    for k, y in ((kl[0:1], 100.0), (kl[1:2], 104.0), (kr[0:1], 102.0)):
        k["startPointX"], k["startPointY"], k["endPointX"], k["endPointY"] = 300.0, y, 400.0, y + 60.0
    dl = np.zeros((2, 32), np.uint8); dr = np.zeros((1, 32), np.uint8)
    dl[0, 0] = 0b111                                                      # distance 3 to the right line
    dl[1, 0] = 0b1                                                        # distance 1
    cfg = oracle.default_config(752, 480)
    disp, le, m = oracle.stereo_lines_tables(cfg, kl, dl, kr, dr, 752, 480)
    assert m.tolist() == [-1, 0]
    cfg.best_lr_matches = 0
    _, _, m = oracle.stereo_lines_tables(cfg, kl, dl, kr, dr, 752, 480)
    assert m.tolist() == [0, 0]


def test_search_by_projection_exclusive_assignment(oracle):
    kp = np.zeros(2, oracle.KEYPOINT_DT)
    kp["x"] = [100.0, 103.0]; kp["y"] = [100.0, 100.0]; kp["octave"] = 0; kp["angle"] = 10.0
    desc = np.zeros((2, 32), np.uint8); desc[1, 0] = 0b1
    q = np.zeros(2, oracle.PROJ_QUERY_DT)
    q["u"] = [101.0, 101.0]; q["v"] = 100.0; q["radius"] = 7.0; q["ur"] = 50.0
    q["min_level"] = -1; q["max_level"] = 1; q["angle"] = 10.0; q["valid"] = 1
    qd = np.zeros((2, 32), np.uint8)
    n, best = oracle.search_by_projection(q, qd, kp, desc, np.full(2, -1, np.float32), (0, 752, 0, 480), False)
    assert best.tolist() == [0, 1] and n == 2      # the second query cannot take keypoint 0 again
    # ORBmatcher.cc:2255-2257: a keypoint is unavailable while the map point it holds has observations.  Keypoint 0 taken before the
    # call: both queries are left with keypoint 1, the first one gets it
    n, best = oracle.search_by_projection(q, qd, kp, desc, np.full(2, -1, np.float32), (0, 752, 0, 480), False, occupied=[1, 0])
    assert best.tolist() == [1, -1] and n == 1
    # ... and a map point WITHOUT observations (UpdateLastFrame's temporal points) does not take its keypoint away: the second query
    # matches keypoint 0 too, nmatches counts both (:2280-2282)
    q3 = q.copy(); q3["valid"] = [3, 1]
    n, best, raw = oracle.search_by_projection(q3, qd, kp, desc, np.full(2, -1, np.float32), (0, 752, 0, 480), False, with_raw=True)
    assert best.tolist() == [0, 0] and raw.tolist() == [0, 0] and n == 2
    # the rotation filter (:2303-2320) works per histogram entry: three queries agree on a rotation of 0 degrees, one (without
    # observations, first on the shared keypoint) is 180 degrees off and is removed — raw keeps it
    # (ComputeThreeMaxima keeps a second bin with at least a tenth of the first one's entries: twelve agree)
    K = 12
    kp4 = np.zeros(K, oracle.KEYPOINT_DT)
    kp4["x"] = 50.0 + 40.0 * np.arange(K); kp4["y"] = 100.0; kp4["angle"] = 10.0
    q4 = np.zeros(K + 1, oracle.PROJ_QUERY_DT)
    q4["u"] = np.concatenate([[50.0], kp4["x"]]); q4["v"] = 100.0; q4["radius"] = 5.0; q4["min_level"] = -1; q4["max_level"] = 1
    q4["angle"] = [190.0] + [10.0] * K; q4["valid"] = [3] + [1] * K
    n, best, raw = oracle.search_by_projection(q4, np.zeros((K + 1, 32), np.uint8), kp4, np.zeros((K, 32), np.uint8), np.full(K, -1, np.float32),
                                               (0, 752, 0, 480), True, with_raw=True)
    assert raw.tolist() == [0] + list(range(K)) and best.tolist() == [-1] + list(range(K)) and n == K


def test_search_local_map_ratio_and_levels(oracle):
    """ORBmatcher.cc:118-138: the ratio test only applies when best and second best are on the same level."""
    kp = np.zeros(3, oracle.KEYPOINT_DT)
    kp["x"] = [100.0, 103.0, 98.0]; kp["y"] = 100.0; kp["octave"] = [1, 1, 0]
    desc = np.zeros((3, 32), np.uint8)
    desc[0, 0] = 0b1111            # distance 4 to a zero query
    desc[1, 0] = 0b11111           # distance 5, same level as keypoint 0
    desc[2, :] = 255               # far away
    ur = np.full(3, -1, np.float32)
    q = np.zeros(1, oracle.PROJ_QUERY_DT)
    q["u"] = 101.0; q["v"] = 100.0; q["radius"] = 7.0; q["min_level"] = 0; q["max_level"] = 1; q["valid"] = 1
    qd = np.zeros((1, 32), np.uint8)
    b = (0, 752, 0, 480)
    n, best = oracle.search_local_map(q, qd, kp, desc, ur, None, b, 0.8)
    assert n == 1 and best.tolist() == [0]          # 4 <= 0.8*5
    n, best = oracle.search_local_map(q, qd, kp, desc, ur, None, b, 0.7)
    assert n == 0 and best.tolist() == [-1]         # 4 > 0.7*5 on the same level
    kp["octave"][1] = 0
    n, best = oracle.search_local_map(q, qd, kp, desc, ur, None, b, 0.7)
    assert n == 1 and best.tolist() == [0]          # different levels: no ratio test
    # occupied keypoints are skipped; the uRight gate uses the query's radius
    n, best = oracle.search_local_map(q, qd, kp, desc, ur, np.array([1, 0, 0], np.uint8), b, 0.7)
    assert best.tolist() == [1]
    ur[:] = [60.0, -1, -1]; q["ur"] = 50.0
    n, best = oracle.search_local_map(q, qd, kp, desc, ur, None, b, 0.7)
    assert best.tolist() == [1]                      # |50-60| > 7 removes keypoint 0
    # one-way matchNNR keeps non-mutual matches that match() would drop
    a = np.zeros((2, 32), np.uint8); t = np.zeros((2, 32), np.uint8)
    a[0, 0] = 0b1; a[1, :4] = 255; t[0, :2] = 255; t[1, :4] = 255
    # a0->t0: 15 < 0.9*31; a1->t1: 0; but t0->a0: 15 !< 0.9*16, so the mutual check of match() drops a0
    n, m = oracle.match_nnr(a, t, 0.9)
    n2, m2 = oracle.match_lines(a, t, 0.9, True)
    assert m.tolist() == [0, 1] and n == 2
    assert m2.tolist() == [-1, 1] and n2 == 1


def test_remap_linear_properties(oracle):
    """cv::remap INTER_LINEAR (stereo_euroc.cc:166): weight blocks, identity, half-pixel, constant-0 border."""
    for fx in range(32):
        for fy in range(32):
            w = oracle.remap_weights(fx, fy)
            assert w.sum() == 32768 and (w >= 0).all() and w.max() <= 32767
            if (fx, fy) != (0, 0):
                assert w.tolist() == [(32 - fx) * (32 - fy) * 32, fx * (32 - fy) * 32, (32 - fx) * fy * 32, fx * fy * 32]
    assert oracle.remap_weights(0, 0).tolist() == [32767, 0, 0, 1]        # 32768 does not fit a short
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (40, 56), dtype=np.uint8)
    xx, yy = np.meshgrid(np.arange(56, dtype=np.float32), np.arange(40, dtype=np.float32))
    assert np.array_equal(oracle.remap_linear(img, xx, yy), img)
    sh = oracle.remap_linear(img, xx + 3, yy - 2)                          # integer shift, zeros shifted in
    assert np.array_equal(sh[2:, :-3], img[:-2, 3:]) and (sh[:2] == 0).all() and (sh[:, -3:] == 0).all()
    half = oracle.remap_linear(img, xx + 0.5, yy)                          # (a + b + 1) >> 1, last column against the 0 border
    exp = (img[:, :-1].astype(int) + img[:, 1:] + 1) >> 1
    assert np.array_equal(half[:, :-1], exp) and np.array_equal(half[:, -1], (img[:, -1].astype(int) + 1) >> 1)
    far = oracle.remap_linear(img, xx + 1000, yy)
    assert (far == 0).all()
    q = oracle.remap_linear(img, xx + np.float32(1 / 64), yy)              # cvRound(x*32 + 0.5): ties to even
    assert np.array_equal(q[:, 0::2][:, :27], img[:, 0::2][:, :27])        # even x: 32x+0.5 -> 32x


def test_bow_vocabulary_descent_and_vector(oracle):
    """DBoW2 transform (TemplatedVocabulary.h:1139-1272) on a hand-made tree: nearest child, first one on ties,
    node at level L - levelsup, stopped words, TF-IDF sums and L1 normalisation in word order."""
    z = np.zeros(32, np.uint8)
    def d(*bits):
        v = z.copy()
        for b in bits:
            v[b >> 3] |= 1 << (b & 7)
        return v
    # root -> A(1), B(2); A -> a0(3), a1(4); B -> b0(5), b1(6)     (file order = breadth first); L = 2
    parent = [0, 0, 1, 1, 2, 2]
    is_leaf = [0, 0, 1, 1, 1, 1]
    desc = [d(), d(0, 1, 2, 3), d(8), d(9), d(0, 1, 2, 3, 8), d(0, 1, 2, 3, 9)]
    weight = [0, 0, 2.0, 0.0, 3.0, 5.0]                                  # a1 is a stopped word
    v = oracle.Vocabulary(2, 2, parent, is_leaf, np.stack(desc), weight)
    f = np.stack([d(8), d(9), d(0, 1, 2, 3, 8), d(0, 1), d(0, 1, 2, 3, 9), d(0, 1, 2, 3, 9)])
    word, wt, node = v.descend(f, levelsup=1)
    assert word.tolist() == [0, 1, 2, 0, 3, 3]                            # d(0,1): tie between A and B -> A (first), then a0/a1 tie -> a0
    assert wt.tolist() == [2.0, 0.0, 3.0, 2.0, 5.0, 5.0]
    assert node.tolist() == [1, 1, 2, 1, 2, 2]                            # level L - 1 = 1
    assert v.descend(f, levelsup=2)[2].tolist() == [0] * 6                # level 0: the root
    words, vals = v.bow_vector(f, levelsup=1)
    assert words.tolist() == [0, 2, 3]                                    # the stopped word does not appear
    assert vals.tolist() == [4.0 / 17.0, 3.0 / 17.0, 10.0 / 17.0]


def test_sincosf_restatement_equals_this_machines_libm(oracle):
    """PLI_PARITY_TRIG_F32_*: the restated cosf / sinf (glibc >= 2.28 algorithm) against the libm of this machine, bit for bit, on
    every 5th float of [2^-13, 2 pi) — the range of the angles on the path — and on a few hand values."""
    import ctypes
    ver = ctypes.CDLL("libc.so.6").gnu_get_libc_version
    ver.restype = ctypes.c_char_p
    major, minor = (int(v) for v in ver().decode().split(".")[:2])
    if (major, minor) < (2, 28):
        import pytest
        pytest.skip("glibc %d.%d has the older cosf" % (major, minor))
    assert oracle.sincosf_selfcheck(0x39000000, 0x40C90FDB, 5) == 0
    assert oracle.glibc_cosf(0.0) == 1.0 and oracle.glibc_sinf(0.0) == 0.0
    assert abs(oracle.glibc_cosf(1.0) - 0.5403023) < 1e-7 and abs(oracle.glibc_sinf(2.5) - 0.5984721) < 1e-7


def test_atan2f_restatement_equals_this_machines_libm(oracle):
    """PLI_PARITY_TRIG_F32_KEYLINE: the restated atan2f (the fdlibm float algorithm of glibc up to 2.40) against the libm of this
    machine, bit for bit, on two million pairs within the range of end-point differences (images up to 2048 px), the axes, x == 1
    and signed zeros, and on a few hand values.  It is not the correctly rounded function: the sample must hold pairs where the
    two differ, or the check would say nothing."""
    assert oracle.atan2f_selfcheck(2000000, 2048.0) == 0
    assert oracle.atan2f_selfcheck(200000, 3.0) == 0
    assert oracle.glibc_atan2f(0.0, 1.0) == 0.0 and oracle.glibc_atan2f(0.0, -1.0) == float(np.float32(np.pi))
    assert oracle.glibc_atan2f(1.0, 0.0) == float(np.float32(np.pi / 2)) and oracle.glibc_atan2f(-1.0, 0.0) == -float(np.float32(np.pi / 2))
    rng = np.random.default_rng(5)
    y, x = rng.uniform(-300, 300, 4000).astype(np.float32), rng.uniform(-300, 300, 4000).astype(np.float32)
    mine = np.array([oracle.glibc_atan2f(float(a), float(b)) for a, b in zip(y, x)], np.float32)
    exact = np.arctan2(y.astype(np.float64), x.astype(np.float64))
    assert np.all(np.abs(mine.astype(np.float64) - exact) <= 1.5 * np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64))
    assert np.any(mine != exact.astype(np.float32))


def test_lsd_f64_pipeline_primitives(oracle):
    """CV_64F Gaussian blur of a constant image is the constant (kernel sums to 1 within rounding); bilinear resize of a linear
    ramp stays linear in the interior with slope 1 / scale."""
    W, H = 40, 30
    cfg = oracle.default_config(W, H, parity_flags=oracle.PARITY_LSD_F64, lsd_nfeatures=0)
    f = oracle.Frame(cfg)
    flat = np.full((H, W), 77, np.uint8)
    f.line_extract(0, flat)
    s = f.lsd_scaled64(0)
    assert s.shape == (36, 48) and np.abs(s - 77.0).max() < 1e-9
    ramp = np.tile((np.arange(W) * 5).astype(np.uint8), (H, 1))
    f.line_extract(0, ramp)
    s = f.lsd_scaled64(0)
    d = np.diff(s[10, 8:40])
    assert np.abs(d - d.mean()).max() < 1e-2 and abs(d.mean() - 5 / 1.2) < 1e-6


# ---------------------------------------------------------------------------------------------
# fisheye stereo (KannalaBrandt8 + ComputeStereoFishEyeMatches), lapping order
# ---------------------------------------------------------------------------------------------
TUMVI_CAM1 = [190.978477, 190.973307, 254.931706, 256.897442, 0.00348238940, 0.000715034845, -0.00205323614, 0.000202936736]
TUMVI_CAM2 = [190.442369, 190.434438, 252.597254, 254.917230, 0.00340031805, 0.00176627874, -0.00266312161, 0.000329951911]


def test_kb8_unproject_project_round_trip(oracle):
    """unproject (Newton, KannalaBrandt8.cpp:103-130) then project (:28-42) returns the pixel; with k = 0 the model is the
    equidistant fisheye r = f * theta."""
    rng = np.random.default_rng(4)
    for rad, phi in zip(rng.uniform(1, 230, 50), rng.uniform(0, 2 * np.pi, 50)):     # (beyond ~290 px the ray is past 90 degrees)
        u, v = TUMVI_CAM1[2] + rad * np.cos(phi), TUMVI_CAM1[3] + rad * np.sin(phi)
        r = oracle.kb8_unproject(TUMVI_CAM1, u, v)
        assert r[2] == 1.0
        uv = oracle.kb8_project(TUMVI_CAM1, r * np.float32(3.0))
        assert np.abs(uv - np.array([u, v], np.float32)).max() < 2e-3
    eq = [100.0, 100.0, 0.0, 0.0, 0, 0, 0, 0]
    uv = oracle.kb8_project(eq, [np.tan(0.5), 0.0, 1.0])
    assert abs(uv[0] - 50.0) < 1e-4 and abs(uv[1]) < 1e-6
    assert oracle.kb8_unproject(eq, 0.0, 0.0).tolist() == [0.0, 0.0, 1.0]              # theta_d <= 1e-8: scale stays 1


from helpers_fisheye import fisheye_tables as _fisheye_tables  # noqa: E402


def test_fisheye_stereo_triangulation(oracle):
    """ComputeStereoFishEyeMatches (Frame.cc:1577-1618): every constructed pair is found, its depth is the z of the 3-D point
    (noise-free: 1e-3 relative), mvRightToLeftMatch is the inverse; a pair without parallax and a point behind the
    camera are refused."""
    a = np.deg2rad(2.0)
    R = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
    t = [0.101, 0.002, -0.001]
    sigma2 = np.array([1.0, 1.44, 2.0736], np.float32)
    P1, kpL, dL, kpR, dR, mono, perm = _fisheye_tables(oracle, TUMVI_CAM1, TUMVI_CAM2, R, t, noise=0.0)
    n, l2r, r2l, depth, p3d = oracle.stereo_fisheye(kpL, dL, mono, kpR, dR, mono, TUMVI_CAM1, TUMVI_CAM2, R, t, sigma2)
    assert n == len(P1) and (l2r[:mono] == -1).all() and (depth[:mono] == -1).all()
    inv = np.empty(len(perm), np.int64); inv[perm - mono] = np.arange(len(perm))        # left i -> right row
    assert np.array_equal(l2r[mono:], mono + inv)
    assert np.array_equal(r2l[l2r[mono:]], np.arange(mono, mono + len(P1)))
    assert np.abs(depth[mono:] / P1[:, 2] - 1).max() < 1e-3 and np.abs(p3d[mono:] - P1).max() < 5e-3
    # with pixel noise most pairs survive the 5.991 sigma^2 gate, not all
    P1, kpL, dL, kpR, dR, mono, perm = _fisheye_tables(oracle, TUMVI_CAM1, TUMVI_CAM2, R, t, noise=1.2, seed=5)
    n2 = oracle.stereo_fisheye(kpL, dL, mono, kpR, dR, mono, TUMVI_CAM1, TUMVI_CAM2, R, t, sigma2)[0]
    assert 0.3 * len(P1) < n2 < len(P1)
    # no parallax (zero baseline): cosParallaxRays > 0.9998 for every pair
    P1, kpL, dL, kpR, dR, mono, perm = _fisheye_tables(oracle, TUMVI_CAM1, TUMVI_CAM1, np.eye(3), [0, 0, 0], noise=0.0)
    assert oracle.stereo_fisheye(kpL, dL, mono, kpR, dR, mono, TUMVI_CAM1, TUMVI_CAM1, np.eye(3), [0, 0, 0], sigma2)[0] == 0
    # fewer than two right candidates: knnMatch returns rows of size < 2 -> nothing
    assert oracle.stereo_fisheye(kpL, dL, mono, kpR[:mono + 1], dR[:mono + 1], mono, TUMVI_CAM1, TUMVI_CAM1, R, t, sigma2)[0] == 0


def test_lapping_order_hand_case(oracle):
    """ORBextractor.cc:1135-1144: lapping keypoints fill the table from the back in visiting order."""
    kp = np.zeros(6, oracle.KEYPOINT_DT)
    kp["x"] = [5, 100, 7, 300, 250, 9]
    order, mono = oracle.lapping_order(kp, 100, 300)
    assert mono == 3 and order.tolist() == [0, 2, 5, 4, 3, 1]
    order, mono = oracle.lapping_order(kp, 0, 0)                      # the rectified pipeline: nothing in [0, 0]
    assert mono == 6 and order.tolist() == [0, 1, 2, 3, 4, 5]


def test_search_local_map_fisheye_partners_and_order(oracle):
    """ORBmatcher.cc:44-214 with F.Nleft != -1, by hand: a left match is also written to the keypoint's right partner, a left
    ratio failure leaves the map point before its right camera is searched, a slot written through a partner is taken for
    the map points that follow, and the partner's slot is overwritten even when it was taken."""
    KP, Q = oracle.KEYPOINT_DT, oracle.PROJ_QUERY_DT
    b = (0, 752, 0, 480)
    kpl = np.zeros(3, KP); kpl["x"] = [100.0, 103.0, 300.0]; kpl["y"] = 100.0; kpl["octave"] = 1
    kpr = np.zeros(2, KP); kpr["x"] = [200.0, 400.0]; kpr["y"] = 100.0; kpr["octave"] = 1
    dl = np.zeros((3, 32), np.uint8); dl[0, 0] = 0b1111; dl[1, 0] = 0b11111; dl[2, :] = 255
    dr = np.zeros((2, 32), np.uint8); dr[1, 0] = 0b1
    l2r = np.array([0, -1, -1], np.int32); r2l = np.array([0, -1], np.int32)

    def query(u, v, valid=1):
        q = np.zeros(1, Q); q["u"] = u; q["v"] = v; q["radius"] = 7.0; q["min_level"] = 0; q["max_level"] = 1; q["valid"] = valid
        return q
    qd = np.zeros((1, 32), np.uint8)
    # left: 4 <= 0.8*5 -> keypoint 0 and its partner right 0; right camera: right 0 is taken now, nothing else near (200,100)
    n, mpl, mpr = oracle.search_local_map_fisheye(query(101, 100), query(200, 100), qd, kpl, dl, None, l2r, kpr, dr, None, r2l, b, 0.8)
    assert n == 2 and mpl.tolist() == [0, -1, -1] and mpr.tolist() == [0, -1]
    # ratio 0.7: the left test fails (4 > 0.7*5, same level) and the map point is left: its right camera is not searched
    n, mpl, mpr = oracle.search_local_map_fisheye(query(101, 100), query(200, 100), qd, kpl, dl, None, l2r, kpr, dr, None, r2l, b, 0.7)
    assert n == 0 and (mpl == -1).all() and (mpr == -1).all()
    # not in view on the left: the right camera takes right 0 and writes its partner left 0 — although left 0 was taken
    n, mpl, mpr = oracle.search_local_map_fisheye(query(101, 100, 0), query(200, 100), qd, kpl, dl, np.array([1, 0, 0], np.uint8), l2r,
                                                  kpr, dr, None, r2l, b, 0.8)
    assert n == 2 and mpl.tolist() == [0, -1, -1] and mpr.tolist() == [0, -1]
    # two map points: the first takes left 0 (+ right 0); the second, same place, finds left 1 only (5 <= 100, second best gone)
    q2l = np.concatenate([query(101, 100), query(101, 100)]); q2r = np.concatenate([query(200, 100, 0), query(200, 100)])
    n, mpl, mpr = oracle.search_local_map_fisheye(q2l, q2r, np.zeros((2, 32), np.uint8), kpl, dl, None, l2r, kpr, dr, None, r2l, b, 0.8)
    assert n == 3 and mpl.tolist() == [0, 1, -1] and mpr.tolist() == [0, -1]
