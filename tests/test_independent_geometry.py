"""The oracle's two camera-geometry statements (oracle.track_queries, oracle.stereo_fisheye) against the float64 restatement of
tests/helpers_geometry.py, which was written from the reference's text in another shape: every exit of both stages is reached
and counted, every deliberately wrong reading (TrackRules / FisheyeRules) is caught by the corpus, and track_queries gets the
hand-worked known answers it never had.  CPU only; tests/test_independent_geometry_gpu.py sends the same tables to the kernels.

Each test prints what it measured (pytest -s shows it; on failure it is in the captured output)."""
import collections
from dataclasses import fields, replace

import numpy as np
import pytest

import helpers_geometry as hg
import helpers_matchers as hm

f32 = np.float32


def oracle_queries(po, b, f):
    c, fr = b["cam"], b["frames"][f - 1]
    return po.track_queries(fr["kp"], fr["depth"], b["poses"][f - 1], b["poses"][f], c.fx, c.fy, c.cx, c.cy, c.bf, c.th, c.mono, b["sf"])


def oracle_search(po, b, f, q):
    last, cur = b["frames"][f - 1], b["frames"][f]
    return po.search_by_projection(q, last["desc"], cur["kp"], cur["desc"], cur["uright"], b["cam"].bounds, False)


def restated_search(b, f, E):
    last, cur = b["frames"][f - 1], b["frames"][f]
    q = hg.queries_from(E, last["kp"])
    return hm.search_by_projection(q, last["desc"], cur["kp"], cur["desc"], cur["uright"], b["cam"].bounds, False)[:2]


def pairs(b):
    return [f for f in range(1, len(b["poses"]))]


def track_deviation(q, E, cam):
    """Worst |oracle - float64| of u, v, ur, radius over the rows both let through: (ulp of float32, pixels).  The ulp is taken at
    the magnitude of the value, and not below the principal-point coordinate that was added to it last."""
    val = (E["label"] == "ok") | (E["label"] == "out_of_image")
    worst_ulp = worst_px = 0.0
    for k, floor in (("u", cam.f("cx")), ("v", cam.f("cy")), ("ur", cam.f("cx")), ("radius", 0.0)):
        with np.errstate(all="ignore"):
            fin = val & np.isfinite(E[k])
        if not fin.any():
            continue
        want = E[k][fin]
        d = np.abs(q[k][fin].astype(np.float64) - want)
        sp = np.spacing(np.maximum(np.abs(want), floor).astype(f32)).astype(np.float64)
        worst_ulp, worst_px = max(worst_ulp, float((d / sp).max())), max(worst_px, float(d.max()))
    return worst_ulp, worst_px


def test_track_oracle_equals_the_restatement(oracle):
    """Labels, level windows and `valid` exactly; u, v, ur, radius within TRACK_TOL_ULP; and the decision itself, made visible by
    the constructed current frames: oracle.search_by_projection on the oracle's queries takes exactly the row the restatement
    expects (by construction, and by helpers_matchers.search_by_projection on the restatement's own queries)."""
    worst_ulp = worst_px = 0.0
    refused = 0
    nrows = 0
    for b in hg.track_corpus():
        refused += b["refused"]
        minx, maxx, miny, maxy = (f32(v) for v in b["cam"].bounds)
        for f in pairs(b):
            E, last = b["E"][f], b["frames"][f - 1]
            q = oracle_queries(oracle, b, f)
            nrows += len(q)
            valid = (E["label"] == "ok") | (E["label"] == "out_of_image")
            assert np.array_equal(q["valid"] > 0, valid), (b["name"], f)
            with np.errstate(invalid="ignore"):
                out = (q["valid"] > 0) & ((q["u"] < minx) | (q["u"] > maxx) | (q["v"] < miny) | (q["v"] > maxy))
            assert np.array_equal(out, E["label"] == "out_of_image"), (b["name"], f)
            assert np.array_equal(q["min_level"][valid], E["lo"][valid]) and np.array_equal(q["max_level"][valid], E["hi"][valid]), (b["name"], f)
            if len(q):
                u, p = track_deviation(q, E, b["cam"])
                worst_ulp, worst_px = max(worst_ulp, u), max(worst_px, p)
                assert u <= hg.TRACK_TOL_ULP, (b["name"], f, u)
            n, best = oracle_search(oracle, b, f, q)
            rn, rbest = restated_search(b, f, E)
            assert np.array_equal(b["expected"][f], rbest), (b["name"], f, "the builder's expectation is not the restatement's")
            assert np.array_equal(best, rbest) and n == rn == int((b["expected"][f] >= 0).sum()), (b["name"], f)
    print("track: %d rows; worst oracle-vs-float64 deviation %.2f ulp, %.3g px (recorded %.3g ulp, %.3g px; tolerance %.3g ulp, "
          "image margin %.3g px, probes at %.3g px); tables refused: %d"
          % (nrows, worst_ulp, worst_px, hg.MEASURED_TRACK_ULP, hg.MEASURED_TRACK_PX, hg.TRACK_TOL_ULP, hg.TRACK_MARGIN["image_px"],
             hg.TRACK_PROBE_PX, refused))
    assert refused == 0
    assert worst_ulp <= hg.MEASURED_TRACK_ULP and worst_px <= hg.MEASURED_TRACK_PX, "the recorded worst deviations are out of date"


def test_track_every_exit_and_window_is_reached():
    labels, windows, roles = collections.Counter(), collections.Counter(), collections.Counter()
    sizes = set()
    for b in hg.track_corpus():
        for f in pairs(b):
            E = b["E"][f]
            labels.update(E["label"].tolist())
            sizes.add(len(E["label"]))
            if len(E["label"]) and (E["label"] == "ok").any():
                windows["forward" if E["forward"] else "backward" if E["backward"] else "mono" if b["cam"].mono else "neutral"] += 1
            cur = b["frames"][f]
            taken = set(b["expected"][f][b["expected"][f] >= 0].tolist())
            roles.update(r[0] for i, r in enumerate(cur["roles"]) if r[0] != "take" or i in taken)
    print("track exits:", dict(labels), "windows:", dict(windows), "rows of the current frames:", dict(roles))
    for k in ("no_depth", "behind", "out_of_image", "ok"):
        assert labels[k] >= 5, (k, labels)
    for k in ("forward", "backward", "neutral", "mono"):
        assert windows[k] >= 1, windows
    for k in ("take", "level", "radius", "uright", "gate"):
        assert roles[k] >= 5, roles
    assert {0, 255, 256, 257} <= sizes


@pytest.mark.parametrize("switch", [f.name for f in fields(hg.TrackRules)])
def test_track_mutation_is_caught(oracle, switch):
    """The restatement with one reading changed disagrees with the oracle somewhere: in a label, a window or, for the searches
    on the constructed current frames, in a match."""
    rules = replace(hg.TREF, **{switch: True})
    caught = []
    for b in hg.track_corpus():
        for f in pairs(b):
            if not len(b["frames"][f - 1]["kp"]):
                continue
            E = hg.track_pair(b, f, rules)
            q = oracle_queries(oracle, b, f)
            valid = (E["label"] == "ok") | (E["label"] == "out_of_image")
            same = np.array_equal(q["valid"] > 0, valid)
            if same:
                same = np.array_equal(q["min_level"][valid], E["lo"][valid]) and np.array_equal(q["max_level"][valid], E["hi"][valid])
            if same:
                same = np.array_equal(oracle_search(oracle, b, f, q)[1], restated_search(b, f, E)[1])
            if not same:
                caught.append("%s/%d" % (b["name"], f))
    print("track mutation %s caught by %d pairs: %s" % (switch, len(caught), caught[:4]))
    assert caught, switch


# ---- hand-worked known answers for track_queries ----
def _kat(oracle, xs, ys, zs, octs, tz, mono=False, Tl=None):
    c = hg.EXACT_CAM
    kp = np.zeros(len(xs), oracle.KEYPOINT_DT)
    kp["x"], kp["y"], kp["octave"] = xs, ys, octs
    T0 = np.eye(4)[:3].astype(f32) if Tl is None else Tl
    T1 = T0.copy()
    T1[2, 3] = f32(T0[2, 3] - f32(tz))
    sf, _ = hm.scale_factors(8, 1.2)
    return oracle.track_queries(kp, np.array(zs, f32), T0, T1, c.fx, c.fy, c.cx, c.cy, c.bf, c.th, mono, sf), sf


def test_track_known_answers_identity_and_windows(oracle):
    """fx = fy = 512, cx = 188, cy = 120, bf = 64 (mb = 0.125), th = 15, identity rotations, power-of-two depths: every step is exact.
    Identity poses: the keypoint projects onto itself and ur = x - bf / z; neutral windows [-1, 1] at octave 0 and [6, 8] at 7."""
    xs, ys, zs, octs = [188.0, 376.0, 100.0, 60.0], [120.0, 0.0, 240.0, 30.0], [2.0, 4.0, 0.5, 16.0], [0, 7, 3, 5]
    q, sf = _kat(oracle, xs, ys, zs, octs, 0.0)
    assert q["valid"].tolist() == [1, 1, 1, 1]
    assert q["u"].tolist() == xs and q["v"].tolist() == ys
    assert q["ur"].tolist() == [188.0 - 32.0, 376.0 - 16.0, 100.0 - 128.0, 60.0 - 4.0]
    assert q["radius"].tolist() == [float(f32(15.0) * sf[o]) for o in octs]
    assert list(zip(q["min_level"].tolist(), q["max_level"].tolist())) == [(-1, 1), (6, 8), (2, 4), (4, 6)]
    # no depth: z <= 0 and NaN
    q, _ = _kat(oracle, xs, ys, [0.0, -1.0, np.nan, 1.0], octs, 0.0)
    assert q["valid"].tolist() == [0, 0, 0, 1]


def test_track_known_answers_forward_backward_are_strict(oracle):
    """tlw = 0, tcw.z = -d: tlc.z == d exactly.  d == mb = 64 / 512 (divided in float): `tlc.z > mb` is strict, the window is the
    neutral one; one ulp above: forward (octave .. top); one ulp below: neutral.  Mirrored for backward (0 .. octave).  bMono with
    tlc.z = 3 m: neutral."""
    mb = f32(64.0) / f32(512.0)
    up, dn = np.nextafter(mb, f32(1)), np.nextafter(mb, f32(0))
    xs, ys, zs, octs = [188.0, 100.0], [120.0, 90.0], [8.0, 4.0], [3, 0]
    neutral, forward, backward = [(2, 4), (-1, 1)], [(3, -1), (0, -1)], [(0, 3), (0, 0)]
    for d, want in ((mb, neutral), (up, forward), (dn, neutral), (-mb, neutral), (-up, backward), (-dn, neutral)):
        q, _ = _kat(oracle, xs, ys, zs, octs, d)
        assert q["valid"].tolist() == [1, 1]
        assert list(zip(q["min_level"].tolist(), q["max_level"].tolist())) == want, d
    q, _ = _kat(oracle, xs, ys, zs, octs, 3.0, mono=True)
    assert list(zip(q["min_level"].tolist(), q["max_level"].tolist())) == neutral
    q, _ = _kat(oracle, xs, ys, zs, octs, 3.0)
    assert list(zip(q["min_level"].tolist(), q["max_level"].tolist())) == forward
    # the point 8 m ahead seen from 3 m further on: u = cx (it is on the axis), ur = cx - bf / 5
    assert q["u"][0] == 188.0 and q["v"][0] == 120.0 and q["ur"][0] == f32(188.0) - f32(64.0) * f32(1.0 / 5.0)


def test_track_known_answer_point_in_the_camera_plane(oracle):
    """x3Dc.z == 0 exactly (depth 0.125, the camera 0.125 further on): invzc = +inf is not `< 0`, so the reference goes on; u is
    +-inf off the axis (out of the image) and NaN on it, and `u < min || u > max` is false for NaN: that query reaches
    GetFeaturesInArea with a NaN centre.  What the oracle does with it, pinned: the query stays valid, its u is NaN, and no keypoint
    can be taken -- not even one with the identical descriptor at the last keypoint's own position."""
    xs, ys, zs, octs = [188.0, 300.0, 188.0], [120.0, 50.0, 200.0], [0.125, 0.125, 0.125], [2, 3, 1]
    q, _ = _kat(oracle, xs, ys, zs, octs, 0.125)
    assert q["valid"].tolist() == [1, 1, 1]
    assert np.isnan(q["u"][0]) and np.isnan(q["v"][0])
    assert q["u"][1] == np.inf and q["v"][1] == -np.inf
    assert np.isnan(q["u"][2]) and q["v"][2] == np.inf
    kp = np.zeros(3, oracle.KEYPOINT_DT)
    kp["x"], kp["y"], kp["octave"] = xs, ys, octs
    desc = hg.code_rows(3)
    for ur in (-1.0, 100.0):
        n, best = oracle.search_by_projection(q, desc, kp, desc, np.full(3, ur, f32), hg.EXACT_CAM.bounds, False)
        assert n == 0 and best.tolist() == [-1, -1, -1]
    # the corpus carries the same rows (exact_tlc_eq_mb); the restatement expects nothing for them either
    b = [b for b in hg.track_corpus() if b["name"] == "exact_tlc_eq_mb"][0]
    assert np.isnan(b["E"][1]["u"][8]) and b["E"][1]["label"][8] == "ok" and b["expected"][1][8] == -1
    assert b["E"][1]["u"][9] == np.inf and b["E"][1]["label"][9] == "out_of_image"


# ---- fisheye ----
def oracle_fisheye(po, T):
    return po.stereo_fisheye(T["kpL"], T["dL"], T["monoL"], T["kpR"], T["dR"], T["monoR"], T["cam1"], T["cam2"], T["R"], T["t"],
                             hg.fisheye_sigma2())


def fisheye_c(got_depth, got_p3d, exp, T):
    """Worst c of |oracle - float64| <= c 2^-23 max(1, z^2 / |t12|) over the accepted rows, depth and p3d."""
    acc = exp["l2r"] >= 0
    if not acc.any():
        return 0.0
    z = exp["depth"][acc]
    unit = hg.EPS32 * np.maximum(1.0, z * z / float(np.linalg.norm(np.asarray(T["t"], np.float64))))
    d = np.maximum(np.abs(got_depth[acc].astype(np.float64) - z), np.abs(got_p3d[acc].astype(np.float64) - exp["p3d"][acc]).max(1))
    return float((d / unit).max())


def test_fisheye_oracle_equals_the_restatement(oracle):
    """Accepted set, l2r, r2l, nmatches exactly; depth and p3d within FISHEYE_TOL_C; the noise-free pairs against the points that
    generated them.  The deviations behind the decided margins are measured again: cosParallaxRays from the oracle's own rays, the
    reprojection error from the oracle's own projection of its own point, the ten float Newton steps against the converged root."""
    worst_cos = worst_px = worst_newton = worst_gen = 0.0
    worst_c = {"default": 0.0, "corner": 0.0}
    refused = 0
    for T in hg.fisheye_corpus():
        exp = T["expect"]
        refused += exp["undecided"]
        n, l2r, r2l, depth, p3d = oracle_fisheye(oracle, T)
        assert n == exp["nmatches"] and np.array_equal(l2r, exp["l2r"]) and np.array_equal(r2l, exp["r2l"]), T["name"]
        assert (depth[l2r < 0] == -1).all() and (p3d[l2r < 0] == 0).all()
        c = fisheye_c(depth, p3d, exp, T)
        worst_c[T["tol"]] = max(worst_c[T["tol"]], c)
        assert c <= hg.FISHEYE_TOL_C[T["tol"]], (T["name"], c)
        ten = hg.run_fisheye(T, newton_steps=10)
        assert ten["labels"] == exp["labels"], T["name"]               # the ten fixed steps decide nothing differently
        R12 = np.asarray(T["R"], f32).reshape(3, 3).astype(np.float64)
        tn = float(np.linalg.norm(np.asarray(T["t"], np.float64)))
        for row, (lab, mg) in enumerate(zip(exp["labels"], exp["margins"])):
            li = T["monoL"] + row
            if "_cos" in mg:
                ri = T["monoR"] + int(np.argsort(hm.hamming(T["dL"][li][None], T["dR"][T["monoR"]:]), kind="stable")[0])
                r1 = oracle.kb8_unproject(T["cam1"], T["kpL"]["x"][li], T["kpL"]["y"][li]).astype(np.float64)
                r2 = oracle.kb8_unproject(T["cam2"], T["kpR"]["x"][ri], T["kpR"]["y"][ri]).astype(np.float64)
                r21 = R12 @ r2
                cosp = r1 @ r21 / (np.linalg.norm(r1) * np.linalg.norm(r21))
                worst_cos = max(worst_cos, abs(cosp - mg["_cos"]) + 2.0 ** -24)
                for cam, kp, k, r in ((T["cam1"], T["kpL"], li, r1), (T["cam2"], T["kpR"], ri, r2)):
                    conv = hg.kb8_unproject64(cam, kp["x"][k], kp["y"][k])
                    fixed = hg.kb8_unproject64(cam, kp["x"][k], kp["y"][k], newton_steps=10)
                    worst_newton = max(worst_newton, float(np.linalg.norm(conv - fixed) / np.linalg.norm(conv)))
            if lab == "ok":
                uv = oracle.kb8_project(T["cam1"], p3d[li]).astype(np.float64)
                e1 = float(np.hypot(uv[0] - float(T["kpL"]["x"][li]), uv[1] - float(T["kpL"]["y"][li])))
                worst_px = max(worst_px, abs(e1 - mg["_e1"]))
                case = T["cases"][row] if row < len(T["cases"]) else None
                if case is not None and case["noise_free"]:
                    # the generating point: the float64 result is off by the rounding of the four pixel coordinates to float32
                    # (2^-16 px each at 256 .. 512 px, 2^-16 / fx as an angle: below one unit for fx > 190), so 4 more units, taken
                    # at the RANGE of the point (the keypoints may be 78 degrees off the axis)
                    rho2 = float(case["P"] @ case["P"])
                    unit = hg.EPS32 * max(1.0, rho2 / tn)
                    gen = float(np.abs(p3d[li].astype(np.float64) - case["P"]).max() / unit)
                    worst_gen = max(worst_gen, gen)
                    assert gen <= hg.FISHEYE_TOL_C["default"] + 4, (T["name"], row, gen)
    print("fisheye: worst oracle-vs-float64 c = %s (recorded %s, tolerance %s), cos %.3g (recorded %.3g), reprojection %.3g px "
          "(recorded %.3g), ten Newton steps vs converged %.3g (recorded %.3g), vs generating points c = %.3g; tables refused: %d"
          % (worst_c, hg.MEASURED_FISHEYE_C, hg.FISHEYE_TOL_C, worst_cos, hg.MEASURED_COS, worst_px, hg.MEASURED_REPROJ_PX, worst_newton,
             hg.MEASURED_NEWTON, worst_gen, refused))
    assert refused == 0
    assert all(worst_c[k] <= hg.MEASURED_FISHEYE_C[k] for k in worst_c) and worst_cos <= hg.MEASURED_COS and worst_px <= hg.MEASURED_REPROJ_PX and \
        worst_newton <= hg.MEASURED_NEWTON, "the recorded worst deviations are out of date"


def test_fisheye_every_exit_is_reached():
    """Every exit of TriangulateMatches and of the loop around it, at least five times -- `z2` included: with the second camera
    turned 90 degrees (rig "wide"), rays that meet in front of camera 1 and behind camera 2 exist and pass the parallax gate."""
    labels, kinds = collections.Counter(), collections.Counter()
    shapes = set()
    for T in hg.fisheye_corpus():
        labels.update(T["expect"]["labels"])
        kinds.update(c["kind"] for c, lab in zip(T["cases"], T["expect"]["labels"]) if lab == "ok")
        shapes.add((len(T["kpL"]) - T["monoL"], min(len(T["kpR"]) - T["monoR"], 3)))
    print("fisheye exits:", dict(labels), "accepted by kind:", dict(kinds))
    for k in ("ratio", "parallax", "z1", "z2", "chi1", "chi2", "depth_floor", "ok"):
        assert labels[k] >= 5, (k, labels)
    assert kinds["centre"] >= 1 and kinds["corner"] >= 5 and kinds["far"] >= 5 and kinds["noise"] >= 5
    assert {63, 64, 65, 0} <= {s[0] for s in shapes} and {0, 1, 2} <= {s[1] for s in shapes}
    main = hg.fisheye_corpus()[0]
    last = len(main["kpL"]) - 1                                      # the repeated left row, more than 64 rows after its twin
    twin = [i for i in range(main["monoL"], last) if main["dL"][i].tobytes() == main["dL"][last].tobytes()]
    assert len(twin) == 1 and last - twin[0] > 64
    e = main["expect"]
    assert e["l2r"][twin[0]] == e["l2r"][last] >= 0 and e["r2l"][e["l2r"][last]] == last


@pytest.mark.parametrize("switch", [f.name for f in fields(hg.FisheyeRules)])
def test_fisheye_mutation_is_caught(oracle, switch):
    rules = replace(hg.FREF, **{switch: True})
    caught = []
    for T in hg.fisheye_corpus():
        n, l2r, r2l, depth, p3d = oracle_fisheye(oracle, T)
        m = hg.run_fisheye(T, rules)
        same = n == m["nmatches"] and np.array_equal(l2r, m["l2r"]) and np.array_equal(r2l, m["r2l"])
        if same:
            same = fisheye_c(depth, p3d, m, T) <= hg.FISHEYE_TOL_C[T["tol"]]
        if not same:
            caught.append(T["name"])
    print("fisheye mutation %s caught by %d tables: %s" % (switch, len(caught), caught[:4]))
    assert caught, switch


def test_fisheye_ratio_known_answers():
    """`d0 < d1 * 0.7` on integers: 7 / 10, 70 / 100, 14 / 20, 35 / 50 fail (7 < 7.0 is false), 6 / 10, 69 / 100, 13 / 20, 3 / 5 pass,
    0 / 0 fails; the integer form used by the restatement is the double comparison for every pair of distances."""
    main = hg.fisheye_corpus()[0]
    lab = main["expect"]["labels"]
    assert [lab[i] == "ratio" for i in range(9)] == [True, False, True, False, True, True, False, True, False]
    for d0 in range(257):
        for d1 in range(d0, 257):
            assert (float(d0) < float(d1) * 0.7) == (10 * d0 < 7 * d1)


def test_fisheye_tables_with_bad_rows_are_refused(oracle):
    """octave outside 0 .. nlevels-1 or a non-finite coordinate, in either table: oracle.stereo_fisheye raises before it indexes
    mvLevelSigma2 (pli_stereo_fisheye_tables returns PLI_ERR_INVALID for the same tables, see the GPU test)."""
    T = [T for T in hg.fisheye_corpus() if T["name"] == "lap65"][0]
    for side, field, value in (("kpL", "octave", 8), ("kpL", "octave", -1), ("kpR", "octave", 8), ("kpR", "octave", -1),
                               ("kpL", "x", np.nan), ("kpL", "y", np.inf), ("kpR", "x", -np.inf), ("kpR", "y", np.nan)):
        bad = dict(T)
        bad[side] = T[side].copy()
        bad[side][field][len(bad[side]) - 1] = value
        with pytest.raises(ValueError):
            oracle_fisheye(oracle, bad)
    assert oracle_fisheye(oracle, T)[0] == T["expect"]["nmatches"]
