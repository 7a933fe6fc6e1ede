"""k_track_queries (through pli_batch_track) and k_fisheye_triangulate (through pli_stereo_fisheye_tables) against the float64
restatement of tests/helpers_geometry.py -- and therefore against the oracle, see test_independent_geometry.py -- on the same
constructed tables, with the constants measured there on the CPU.

pli_batch_track keeps its queries to itself, so every decision of the projection is made visible through best_idx2: frame f of a
batch is the probe table that helpers_geometry builds from the float64 projection of frame f - 1 (one row to take per query
that gets through, decoys with a better descriptor that only a wrong window, radius, uRight gate, pose row or gate admits).
The records are written on the host from fe.layout and handed over as a caller-owned device table; nothing is extracted."""
import ctypes as C

import numpy as np
import pytest

import helpers_geometry as hg

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from oracle import pyoracle
    from pli_slam_amd import capi
    from pli_slam_amd.frontend import Frontend
    pyoracle.lib()

    class G:
        pass
    g = G()
    g.capi, g.Frontend, g.torch, g.po = capi, Frontend, torch, pyoracle
    return g


def host_table(fe, frames):
    """Frame records of fe.layout: counts (left keypoints only, no lines), left keypoints, descriptors, uright, depth."""
    Y = fe.layout
    rb = int(Y.record_bytes)
    tab = np.zeros(rb * len(frames), np.uint8)
    for f, fr in enumerate(frames):
        n = len(fr["kp"])
        kp = fr["kp"]
        assert n <= fe.kp_cap and len(fr["desc"]) == len(fr["uright"]) == len(fr["depth"]) == n
        assert np.isfinite(kp["x"]).all() and np.isfinite(kp["y"]).all() and ((kp["octave"] >= 0) & (kp["octave"] < fe.cfg.orb_nlevels)).all()
        assert ((kp["x"] >= 0) & (kp["x"] <= fe.cfg.width) & (kp["y"] >= 0) & (kp["y"] <= fe.cfg.height)).all()
        rec = tab[f * rb:(f + 1) * rb]
        rec[Y.off_counts:Y.off_counts + 32].view(np.int32)[0] = n
        for off, arr in ((Y.off_kp[0], fr["kp"]), (Y.off_desc[0], fr["desc"]), (Y.off_uright, fr["uright"].astype(f32)),
                         (Y.off_depth, fr["depth"].astype(f32))):
            b = np.ascontiguousarray(arr).view(np.uint8).ravel()
            rec[off:off + b.size] = b
    return tab


def run_track(g, fe, b):
    torch, c = g.torch, b["cam"]
    F = len(b["frames"])
    tp = g.capi.TrackParams(fx=c.fx, fy=c.fy, cx=c.cx, cy=c.cy, bf=c.bf, th=c.th, min_x=c.min_x, max_x=c.max_x, min_y=c.min_y,
                            max_y=c.max_y, mono=int(c.mono), check_orientation=0, nnr_lines=0.9, reserved=0)
    tl = fe.track_layout()
    d_table = torch.from_numpy(host_table(fe, b["frames"])).cuda()
    d_poses = torch.from_numpy(np.ascontiguousarray(b["poses"], f32).reshape(-1)).cuda()
    d_track = torch.full((F * int(tl.record_bytes),), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    fe.batch_track_device(F, d_table.data_ptr(), d_poses.data_ptr(), tp, d_track.data_ptr())
    fe.sync()
    track = d_track.cpu().numpy()
    return [None] + [fe.parse_track(track, f) for f in range(1, F)]


def test_track_projection_on_constructed_batches(gpu):
    """best_idx2 of every pair of every batch equals the restatement's expectation and the oracle's; counts[0] and counts[1] too.
    The batches: three pairs with three motion cases and a rotation each in ONE call (a wrong pose row shows), last frames of
    255 / 256 / 257 rows (the 256-thread block of k_track_queries), an empty last frame, a monocular batch, and the exact tables
    (tlc.z ON +-mb and one ulp either side, projections ON mnMaxX / mnMinY, x3Dc.z == 0 with u = NaN and u = inf)."""
    g = gpu
    sf, _ = hg.hm.scale_factors(8, 1.2)
    cfg = g.capi.default_config(376, 240, orb_nfeatures=300, lsd_nfeatures=20, max_frames=4)
    fe = g.Frontend(cfg)
    assert fe.kp_cap >= 257 and cfg.orb_nlevels == 8 and cfg.orb_scale_factor == f32(1.2)
    seen = set()
    for b in hg.track_corpus():
        assert np.array_equal(b["sf"], sf)
        got = run_track(g, fe, b)
        c = b["cam"]
        for f in range(1, len(b["frames"])):
            last, cur, E = b["frames"][f - 1], b["frames"][f], b["E"][f]
            q = g.po.track_queries(last["kp"], last["depth"], b["poses"][f - 1], b["poses"][f], c.fx, c.fy, c.cx, c.cy, c.bf, c.th,
                                   c.mono, sf)
            on, obest = g.po.search_by_projection(q, last["desc"], cur["kp"], cur["desc"], cur["uright"], c.bounds, False)
            tr = got[f]
            want = b["expected"][f]
            assert tr["counts"][0] == len(last["kp"]), (b["name"], f, tr["counts"])
            bad = np.flatnonzero(tr["best"] != want)
            assert bad.size == 0, "%s pair %d: best_idx2 differs from the float64 restatement at last keypoints %s: got %s, want %s (%s)" % (
                b["name"], f, bad[:5], tr["best"][bad[:5]], want[bad[:5]], E["label"][bad[:5]])
            assert np.array_equal(tr["best"], obest), (b["name"], f, "differs from the oracle")
            assert tr["counts"][1] == on == int((want >= 0).sum()), (b["name"], f, tr["counts"], on)
            if (E["label"] == "ok").any():
                seen.add("forward" if E["forward"] else "backward" if E["backward"] else "mono" if c.mono else "neutral")
            seen.update(E["label"].tolist())
            seen.add(len(last["kp"]))
    assert {"forward", "backward", "neutral", "mono", "ok", "behind", "no_depth", "out_of_image", 0, 255, 256, 257} <= seen
    fe.close()


def fisheye_context(g):
    cfg = g.capi.default_config(512, 512, orb_nfeatures=500, lsd_nfeatures=0)
    fe = g.Frontend(cfg)
    sigma2 = g.po.Frame(g.po.Config.from_buffer_copy(bytes(cfg))).level_sigma2()
    assert np.array_equal(sigma2, hg.fisheye_sigma2())
    return fe, sigma2


def test_fisheye_triangulation_on_the_corpus(gpu):
    """nmatches, l2r, r2l exactly as the restatement decides them; depth and p3d within the tolerance measured on the CPU
    (FISHEYE_TOL_C) and bit-equal to the oracle.  The tables: every exit of TriangulateMatches, lapping areas of 63 / 64 / 65 left
    rows (the 64-thread block), 0 / 1 / 2 right lapping rows, an empty left lapping area, two left rows with one descriptor more
    than 64 rows apart (the atomicMax across blocks), keypoints at the principal point and towards the corner, four rigs."""
    g = gpu
    fe, sigma2 = fisheye_context(g)
    worst = {"default": 0.0, "corner": 0.0}
    for T in hg.fisheye_corpus():
        exp = T["expect"]
        got = fe.stereo_fisheye_tables(T["kpL"], T["dL"], T["monoL"], T["kpR"], T["dR"], T["monoR"], T["cam1"], T["cam2"], T["R"], T["t"])
        n, l2r, r2l, depth, p3d = got
        bad = np.flatnonzero(l2r != exp["l2r"])
        assert bad.size == 0, "%s: accept / reject differs from the float64 restatement at left rows %s (%s)" % (
            T["name"], bad[:5], [exp["labels"][i - T["monoL"]] for i in bad[:5] if i >= T["monoL"]])
        assert n == exp["nmatches"] and np.array_equal(r2l, exp["r2l"]), T["name"]
        acc = exp["l2r"] >= 0
        assert (depth[~acc] == -1).all() and (p3d[~acc] == 0).all(), T["name"]
        if acc.any():
            z = exp["depth"][acc]
            unit = hg.EPS32 * np.maximum(1.0, z * z / float(np.linalg.norm(np.asarray(T["t"], np.float64))))
            d = np.maximum(np.abs(depth[acc].astype(np.float64) - z), np.abs(p3d[acc].astype(np.float64) - exp["p3d"][acc]).max(1))
            c = float((d / unit).max())
            worst[T["tol"]] = max(worst[T["tol"]], c)
            assert c <= hg.FISHEYE_TOL_C[T["tol"]], (T["name"], c)
        o = g.po.stereo_fisheye(T["kpL"], T["dL"], T["monoL"], T["kpR"], T["dR"], T["monoR"], T["cam1"], T["cam2"], T["R"], T["t"], sigma2)
        assert n == o[0] and np.array_equal(l2r, o[1]) and np.array_equal(r2l, o[2]), T["name"]
        assert depth.tobytes() == o[3].tobytes() and p3d.tobytes() == o[4].tobytes(), T["name"]
    print("fisheye kernel vs float64: worst c = %s (tolerance %s)" % (worst, hg.FISHEYE_TOL_C))
    fe.close()


def test_fisheye_tables_with_bad_rows_are_refused(gpu):
    """An octave outside 0 .. nlevels-1 or a non-finite coordinate, in either table: PLI_ERR_INVALID with a message, the output
    arrays untouched (the call returns before the kernels that would index mvLevelSigma2 with it)."""
    g = gpu
    fe, _ = fisheye_context(g)
    T = [T for T in hg.fisheye_corpus() if T["name"] == "lap65"][0]
    ptr = g.capi.ptr
    c1, c2 = np.ascontiguousarray(T["cam1"], f32), np.ascontiguousarray(T["cam2"], f32)
    R, t = np.ascontiguousarray(T["R"], f32).reshape(9), np.ascontiguousarray(T["t"], f32)
    for side, field, value in (("kpL", "octave", 8), ("kpL", "octave", -1), ("kpR", "octave", 8), ("kpR", "octave", -1),
                               ("kpL", "x", np.nan), ("kpL", "y", np.inf), ("kpR", "x", -np.inf), ("kpR", "y", np.nan)):
        tabs = {k: np.ascontiguousarray(T[k]).copy() for k in ("kpL", "kpR", "dL", "dR")}
        tabs[side][field][len(tabs[side]) - 1] = value
        nl, nr = len(tabs["kpL"]), len(tabs["kpR"])
        l2r, r2l = np.full(nl, 77, np.int32), np.full(nr, 77, np.int32)
        depth, p3d = np.full(nl, 77, f32), np.full((nl, 3), 77, f32)
        nm = C.c_int32(77)
        st = fe.L.pli_stereo_fisheye_tables(fe.h, ptr(tabs["kpL"]), ptr(tabs["dL"]), nl, T["monoL"], ptr(tabs["kpR"]), ptr(tabs["dR"]), nr,
                                            T["monoR"], ptr(c1), ptr(c2), ptr(R), ptr(t), ptr(l2r), ptr(r2l), ptr(depth), ptr(p3d),
                                            C.byref(nm))
        assert st == -1, (side, field, value, st)                       # PLI_ERR_INVALID
        assert b"octave" in fe.L.pli_last_error()
        assert nm.value == 0 and (l2r == 77).all() and (r2l == 77).all() and (depth == 77).all() and (p3d == 77).all()
        with pytest.raises(g.capi.PliError):
            fe.stereo_fisheye_tables(tabs["kpL"], tabs["dL"], T["monoL"], tabs["kpR"], tabs["dR"], T["monoR"], T["cam1"], T["cam2"], T["R"], T["t"])
    # the context is as usable as before
    got = fe.stereo_fisheye_tables(T["kpL"], T["dL"], T["monoL"], T["kpR"], T["dR"], T["monoR"], T["cam1"], T["cam2"], T["R"], T["t"])
    assert got[0] == T["expect"]["nmatches"] > 0
    fe.close()
