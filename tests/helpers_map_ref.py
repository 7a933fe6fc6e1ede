"""The local-map pin's corpus and fixtures: Frame::isInFrustum, Frame::isInFrustum_l, MapPoint::PredictScale(dist, Frame*), the two
Get*DistanceInvariance, LocalMapping::CreateNewMapPoints (one camera; with ComputeF12 and KeyFrame::UnprojectStereo) and MapPoint /
MapLine::ComputeDistinctiveDescriptors of the reference, cut out of its sources at build time
and compiled where they lie into oracle/_ref/pli_ref_map (oracle/Makefile: ref_map; the stand-in is
oracle/ref_recipe/map_shim/pli_map_shim.hpp), run over the scenes, constructed rows and hand groups the CPU tests of
pli_search_local_points, pli_search_local_lines, pli_create_new_map_points and pli_distinctive_descriptors already have.

  CASES            the named cases: the input arrays of one driver call, and what the restatement and the device make of them
  run_reference    one call of pli_ref_map as a child process
  save_fixture / load_fixture    tests/golden/map_ref/<case>.npz: "in/<array>" and "out/call/<array>" (helpers_match_ref's format)

tools/gen_map_ref.py writes the fixtures; tests/test_ref_pin_map.py and tests/test_ref_pin_map_gpu.py read them.  Nothing here reads
the reference tree; run_reference needs the program oracle/Makefile built from it.

The map points of a case carry mfMinDistance / mfMaxDistance themselves: the reference's getters return 0.8f * mfMinDistance and
1.2f * mfMaxDistance (MapPoint.cc:437-447), and the pli_fuse_point rows every yardstick and the device take are derived from them
the same way (point_rows), as the adapter derives them from the getters.
"""
import math
import os
from collections import Counter

import numpy as np

import helpers_distinctive as HD
import helpers_local_map as lm
import helpers_match_ref as HM
import helpers_matchers as hm
import helpers_new_map_points as NP
from test_fuse_search_cpu import CAM, FUSE_POINT_DT, INV_SIGMA2, NLEVELS, SCALE, SF, level_ratio

ROOT = HM.ROOT
GOLD_DIR = os.path.join(ROOT, "tests", "golden", "map_ref")
REF_EXE = os.path.join(ROOT, "oracle", "_ref", "pli_ref_map")
f32, f64 = np.float32, np.float64
CALL = "call"
SEED = 21
_FIX = {}


def run_reference(bag, exe=None):
    return HM.run_reference(bag, exe or REF_EXE)


def fixture_path(name):
    return os.path.join(GOLD_DIR, name + ".npz")


def save_fixture(name, arrays, results):
    """helpers_match_ref.save_fixture's deterministic bytes, in this pin's folder."""
    keep = HM.GOLD_DIR
    HM.GOLD_DIR = GOLD_DIR
    try:
        HM.save_fixture(name, arrays, results)
    finally:
        HM.GOLD_DIR = keep


def load_fixture(name, call=CALL):
    """-> (arrays, results of the one call); read once, left unchanged.  call "f64": what the generator added from the float64
    statement (NewPointsCase.judge), not an answer of the reference."""
    if name not in _FIX:
        z = np.load(fixture_path(name))
        arrays, res = {}, {}
        for key in z.files:
            parts = key.split("/")
            if parts[0] == "in":
                arrays[parts[-1]] = z[key]
            else:
                res.setdefault(parts[1], {})[parts[-1]] = z[key]
        for a in list(arrays.values()) + [v for r in res.values() for v in r.values()]:
            a.setflags(write=False)
        _FIX[name] = (arrays, res)
    return _FIX[name][0], _FIX[name][1].get(call, {})


def _fn(name):
    return np.frombuffer(name.encode(), np.uint8).copy()


def _frame_bag(a):
    pose = a["pose"]
    return {"f_cam": a["cam"], "f_R": pose[:9].copy(), "f_t": pose[9:12].copy(), "f_Ow": pose[12:15].copy()}


class Case:
    fn = None
    group = None                                  # the key of BY_FN where it is not fn (two forms of one driver function)

    def __init__(self, name, arrays, tags=()):
        self.name, self._arrays, self.tags, self.calls = name, arrays, tuple(tags), [CALL]

    def arrays(self):
        if callable(self._arrays):
            self._arrays = self._arrays()
        return self._arrays


# =========================================================================================================== isInFrustum + search
def predict_scale_ref(ratio):
    """MapPoint::PredictScale(dist, Frame*) (MapPoint.cc:466-481) as the reference's translation unit compiles it: under its
    `using namespace std` the log of the float ratio is logf (oracle/_ref/map_cut.o imports logf and no log), the quotient by
    mfLogScaleFactor a float division, ceil of that float.  logf is taken here as the correctly rounded logarithm; the fixture
    points_level_bounds holds that to the compiled code on both sides of every level bound.  (test_fuse_search_cpu.predict_scale
    takes the logarithm in double: one level more at ratio == 1.2f, see level_ratio_ref.)"""
    ratio = f32(ratio)
    if not ratio > 0:
        return 0
    if math.isinf(ratio):
        return NLEVELS - 1                        # (undefined in the reference: _infinite_ratio)
    n = math.ceil(float(f32(f32(math.log(float(ratio))) / HM.LOGSF)))
    return 0 if n < 0 else NLEVELS - 1 if n >= NLEVELS else int(n)


_LR = {}


def level_ratio_ref():
    """The level_ratio table of pli_search_local_points for predict_scale_ref, as the adapter's localMapLevelRatio builds it from the
    host's own expression.  It differs from test_fuse_search_cpu.level_ratio() in one entry by one ulp: ratio == 1.2f is level 1
    here (logf(1.2f) / mfLogScaleFactor is 1 exactly) and level 2 there."""
    if "t" not in _LR:
        from pli_slam_amd.frontend import fuse_level_ratio
        _LR["t"] = fuse_level_ratio(NLEVELS, SCALE, predict_scale_ref)
    return _LR["t"]


def point_rows(a):
    """The pli_fuse_point rows and descriptors of a points case: valid 0 for a point the loop skips (bad, or seen in this frame
    without a view), PLI_LOCAL_STORED_VIEW for one seen in this frame that still holds mbTrackInView."""
    n = len(a["mp_bad"])
    pts = np.zeros(n, FUSE_POINT_DT)
    pts["pos"], pts["normal"] = a["mp_pos"], a["mp_normal"]
    pts["max_dist"] = a["mp_max_dist"]
    pts["min_dist_inv"] = (f32(0.8) * a["mp_min_dist"]).astype(f32)
    pts["max_dist_inv"] = (f32(1.2) * a["mp_max_dist"]).astype(f32)
    t = a["mp_track"]
    for i in range(n):
        if a["mp_bad"][i]:
            pts["valid"][i] = 0
        elif a["mp_seen"][i]:
            pts["valid"][i] = lm.STORED_VIEW if t[i, 0] else 0
            if t[i, 0]:
                pts["pos"][i], pts["normal"][i] = t[i, 1:4], t[i, 4:7][[0, 2, 1]]      # (depth, view_cos, level)
        else:
            pts["valid"][i] = 1
    return pts, a["mp_desc"]


def points_arrays(pts, descs, pose, kp, desc, ur, occ, th=1.0, far=False, th_far=0.0, nnratio=0.8, cam=CAM, rng=None):
    """pts: FUSE_POINT_DT rows of helpers_local_map (valid 0 / 1 / STORED_VIEW).  max_dist is mfMaxDistance; a row whose scene gave it
    another max_dist_inv / min_dist_inv than the getters' gets the mfMaxDistance / mfMinDistance that the bound came from."""
    n = len(pts)
    rng = rng or np.random.default_rng(n)
    mx = pts["max_dist"].astype(f32).copy()
    off = pts["max_dist_inv"].astype(f64) < 1.19 * pts["max_dist"].astype(f64)            # the scene's "too far" rows
    mx[off] = (pts["max_dist_inv"][off].astype(f64) / 1.2).astype(f32)
    mn = (pts["min_dist_inv"].astype(f64) / 0.8).astype(f32)
    stored = pts["valid"] == lm.STORED_VIEW
    track = np.zeros((n, 8), f32)
    track[stored, 0] = 1
    track[stored, 1:4] = pts["pos"][stored]
    track[stored, 4], track[stored, 6], track[stored, 5] = pts["normal"][stored].T
    skip = pts["valid"] == 0
    bad = skip & (rng.random(n) < 0.5)                                                    # a skipped row is bad or seen, by turns
    seen = (skip & ~bad) | stored
    pos, normal = pts["pos"].astype(f32).copy(), pts["normal"].astype(f32).copy()
    pos[stored], normal[stored] = 0, 0
    return {"params": np.array([nnratio, th, far, th_far], f64), "pose": np.asarray(pose, f32), "cam": HM.cam10(cam),
            "mp_pos": pos, "mp_normal": normal, "mp_desc": np.asarray(descs, np.uint8).reshape(n, 32),
            "mp_bad": bad.astype(np.uint8), "mp_seen": seen.astype(np.uint8), "mp_min_dist": mn, "mp_max_dist": mx, "mp_track": track,
            "cur_x": kp["x"].astype(f32), "cur_y": kp["y"].astype(f32), "cur_octave": kp["octave"].astype(np.int32),
            "cur_angle": kp["angle"].astype(f32), "cur_desc": np.asarray(desc, np.uint8).reshape(len(kp), 32),
            "cur_uright": np.asarray(ur, f32), "cur_occ": np.zeros(len(kp), np.uint8) if occ is None else np.asarray(occ, np.uint8)}


class PointsCase(Case):
    """Tracking.cc:3809-3827 and the search of :3854 on one frame."""
    fn = "frustum_points"
    undefined_level = ()                          # rows whose mnTrackScaleLevel the reference leaves undefined (_infinite_ratio)

    def bag(self, a):
        bag = {"fn": _fn(self.fn), "params": a["params"], "f_sf": SF.astype(f32), "f_sigma2": HM.SIGMA2, "f_inv_sigma2": INV_SIGMA2.astype(f32),
               "f_logsf": np.array([HM.LOGSF], f32), "f_x": a["cur_x"], "f_y": a["cur_y"], "f_octave": a["cur_octave"], "f_angle": a["cur_angle"],
               "f_desc": a["cur_desc"], "f_uright": a["cur_uright"], "f_occ": a["cur_occ"]}
        bag.update(_frame_bag(a))
        bag.update({k: v for k, v in a.items() if k.startswith("mp_")})
        return bag

    def kp(self, a):
        return HM.keypoints(a["cur_x"], a["cur_y"], a["cur_octave"], a["cur_angle"])

    def expected(self, a, res):
        """-> (view records, best_idx2, n_in_view, nmatches) in pli_search_local_points' terms.  A point the loop visits and refuses
        keeps what it held before in mTrackProjXR, mTrackDepth, mnTrackScaleLevel and mTrackViewCos: zero in every case here."""
        pts, _ = point_rows(a)
        n = len(pts)
        view = np.zeros(n, lm.LOCAL_VIEW_DT)
        t = res["track"]
        live = pts["valid"] == 1
        for name, col in (("in_view", 0), ("proj_x", 1), ("proj_y", 2), ("proj_xr", 3), ("depth", 4), ("level", 5), ("view_cos", 6)):
            view[name][live] = t[live, col]
        assert np.array_equal(t[~live], a["mp_track"][~live])                             # a skipped point keeps every field
        best = np.full(n, -1, np.int32)
        rows = res["frame_mp"]
        held = np.flatnonzero((rows >= 0) & (rows < n))
        best[rows[held]] = held
        return view, best, int(res["n_to_match"][0]), int(res["ret"][0])

    def restate(self, a, misread=(), exits=None):
        pts, descs = point_rows(a)
        nn, th, far, th_far = a["params"]
        view, best, nv, nm, _ = lm.search_local_points(pts, descs, a["pose"], self.kp(a), a["cur_desc"], a["cur_uright"], a["cur_occ"] == 1,
                                                       HM.cam_of(a["cam"]), th=th, far_points=bool(far), th_far=th_far, nnratio=nn,
                                                       exits=exits, misread=tuple(m for m in misread if m != "level_log_double"),
                                                       lr=level_ratio() if "level_log_double" in misread else level_ratio_ref())
        return view, best, nv, nm

    def device(self, fe, a):
        pts, descs = point_rows(a)
        nn, th, far, th_far = a["params"]
        return fe.search_local_points(pts, descs, a["pose"], HM.cam_of(a["cam"]), self.kp(a), a["cur_desc"], a["cur_uright"], th=th,
                                      far_points=bool(far), th_far=th_far, nnratio=nn, cur_occupied=(a["cur_occ"] == 1).astype(np.uint8),
                                      level_ratio=level_ratio_ref())

    def same(self, want, got):
        view = got[0].astype(lm.LOCAL_VIEW_DT)
        for i in self.undefined_level:
            view["level"][i] = want[0]["level"][i]
        return (lm.canonical(want[0]) == lm.canonical(view) and want[1].tobytes() == np.asarray(got[1], np.int32).tobytes()
                and (int(want[2]), int(want[3])) == (int(got[2]), int(got[3])))


def _scene_points(nq, th, far, stored=False):
    def make():
        pose, pts, descs, kp, desc, ur, occ = lm.point_scene(SEED, 300, 300)
        pts, descs = pts[:nq].copy(), descs[:nq].copy()
        if stored:                                   # every fifth row a stored view aimed at a keypoint or at nothing (test_local_map_gpu.py)
            rng = np.random.default_rng(5)
            for i in range(0, nq, 5):
                j = int(rng.integers(0, 300))
                aimed = rng.random() < 0.7
                x, y = (kp["x"][j] + rng.uniform(-2, 2), kp["y"][j] + rng.uniform(-2, 2)) if aimed else rng.uniform(-50, 800, 2)
                pts[i:i + 1] = lm.stored_view(x, y, x - rng.uniform(1, 30), rng.uniform(1, 20), rng.uniform(0.99, 1.0), int(kp["octave"][j]))
                descs[i] = desc[j]
        occ = np.where(occ != 0, 1 + (np.arange(len(occ)) % 2), 0)                        # held rows: with observations and without
        return points_arrays(pts, descs, pose, kp, desc, ur, occ, th=th, far=far, th_far=12.0)
    return make


def _ulps(x, k):
    return (np.array([x], f32).view(np.int32) + k).view(f32)[0]


def point_coordinate_on(target, f, c, z, divide=True):
    """A camera coordinate x with fx * x / z + cx (Pinhole::project) or fx * x * invz + cx (isInFrustum_l) equal to target exactly."""
    invz = f32(f32(1.0) / z)
    x0 = f32((float(target) - float(c)) * float(z) / float(f))
    for k in range(-64, 65):
        x = _ulps(x0, k) if x0 != 0 else f32(0.0)
        u = f32(f32(f32(f * x) / z) + c) if divide else f32(f32(f32(f * x) * invz) + c)
        if u == target:
            return x
    return None


def points_on_the_bounds(cam=CAM, divide=True, seed=5):
    """Five camera points (identity pose): one on each image bound with the other coordinate inside, one on the far corner."""
    rng = np.random.default_rng(seed)
    out = []
    targets = [(cam.min_x, None), (cam.max_x, None), (None, cam.min_y), (None, cam.max_y), (cam.max_x, cam.max_y)]
    for tu, tv in targets:
        for _ in range(400):
            z = f32(rng.uniform(1.0, 8.0))
            x = point_coordinate_on(tu, cam.fx, cam.cx, z, divide) if tu is not None else f32(rng.uniform(-0.3, 0.3))
            y = point_coordinate_on(tv, cam.fy, cam.cy, z, divide) if tv is not None else f32(rng.uniform(-0.2, 0.2))
            if x is not None and y is not None:
                out.append((x, y, z))
                break
        else:
            raise AssertionError("no point on the bound")
    return np.array(out, f32)


def _dist_on_the_bound(which, seed=11):
    """A point and an mfMinDistance / mfMaxDistance with 0.8f * mfMinDistance == dist resp. 1.2f * mfMaxDistance == dist exactly."""
    rng = np.random.default_rng(seed)
    for _ in range(2000):
        pos = np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.3, 0.3), rng.uniform(2, 6)]).astype(f32)
        dist = lm._norm3(pos)
        k = f32(0.8) if which == "min" else f32(1.2)
        m0 = f32(float(dist) / float(k))
        for s in range(-4, 5):
            m = _ulps(m0, s)
            if f32(k * m) == dist:
                return pos, m
    raise AssertionError("no distance on the bound")


def _constructed_points():
    rows = [lm.one_point(p, normal=np.asarray(p, f64) / np.linalg.norm(np.asarray(p, f64))) for p in points_on_the_bounds()]
    rows += [lm.one_point((0.0, 0.0, 0.0)), lm.one_point((1.0, 0.0, 0.0)), lm.one_point((-1.0, 0.0, 0.0)),
             lm.one_point((0.1, 0.1, -1e-6)), lm.point_where_the_angle_tests_disagree()]
    pts = np.concatenate(rows)
    extra = []
    for which in ("min", "max"):
        pos, m = _dist_on_the_bound(which)
        P = lm.one_point(pos, normal=pos.astype(f64) / np.linalg.norm(pos.astype(f64)))
        extra.append((P, which, m))
    kp = np.zeros(4, hm.KEYPOINT_DT)
    kp["x"], kp["y"] = (0.0, 100.0, CAM.max_x - 7, CAM.max_x), (0.0, 100.0, CAM.max_y - 6, CAM.max_y)
    kp["octave"] = (NLEVELS - 1, NLEVELS - 1, 0, 0)
    pts = np.concatenate([pts] + [e[0] for e in extra])
    a = points_arrays(pts, np.zeros((len(pts), 32), np.uint8), lm.IDENTITY, kp, np.zeros((4, 32), np.uint8), np.full(4, -1, f32), None, th=3.0)
    # the constructed rows have no range gate (mfMinDistance 0, mfMaxDistance huge) and their own level distance; points_arrays
    # took max_dist for mfMaxDistance, which would put the range gate at 1.2 * dist: still open, and the level stays the row's
    n0 = len(rows)
    a["mp_max_dist"][5] = 0            # the point at the camera centre: mfMaxDistance / dist is 0 / 0, level 0 (see _infinite_ratio)
    for j, (P, which, m) in enumerate(extra):
        if which == "min":
            a["mp_min_dist"][n0 + j] = m
        else:
            a["mp_max_dist"][n0 + j] = m
    return a


def _infinite_ratio():
    """A point at the camera centre with mfMaxDistance > 0: dist is 0, the projection NaN (it stays in view and takes no keypoint),
    and PredictScale converts ceil(log(+inf) / mfLogScaleFactor) to int, which C++ leaves undefined.  The fixture records what the
    build that wrote it returned; PointsCase.undefined_level names the row, and the level of that row alone is not compared."""
    pts = np.concatenate([lm.one_point((0.0, 0.0, 0.0)), lm.one_point((0.1, -0.1, 3.0), normal=(0.0, 0.0, 1.0))])
    kp = np.zeros(2, hm.KEYPOINT_DT)
    kp["x"], kp["y"], kp["octave"] = (0.0, 300.0), (0.0, 200.0), (0, NLEVELS - 1)
    return points_arrays(pts, np.zeros((2, 32), np.uint8), lm.IDENTITY, kp, np.zeros((2, 32), np.uint8), np.full(2, -1, f32), None)


def _level_bounds():
    """For every level bound two points, mfMaxDistance / dist on the last float of the lower level and on the first of the upper."""
    rows, mxs = [], []
    for t in level_ratio_ref():
        for ratio in (t, _ulps(t, 1)):
            for step in range(4096):                                     # not every quotient exists for one dist: step the depth
                pos = np.array([0.1, -0.1, _ulps(3.0, step)], f32)
                dist = lm._norm3(pos)
                m0 = f32(float(ratio) * float(dist))
                hit = [m for m in (_ulps(m0, k) for k in range(-4, 5)) if f32(m / dist) == ratio]
                if hit:
                    break
            rows.append(lm.one_point(pos, normal=(0.0, 0.0, 1.0)))
            mxs.append(hit[0])
    pts = np.concatenate(rows)
    pts["max_dist"] = mxs
    pts["max_dist_inv"] = 1.2 * pts["max_dist"]
    kp = np.zeros(1, hm.KEYPOINT_DT)
    return points_arrays(pts, np.zeros((len(pts), 32), np.uint8), lm.IDENTITY, kp, np.zeros((1, 32), np.uint8), np.full(1, -1, f32), None)


POINT_SIZES = ((0, 1.0, False), (1, 3.0, False), (63, 1.0, True), (64, 3.0, True), (65, 1.0, False), (257, 3.0, True))


# ============================================================================================================== isInFrustum_l
def lines_arrays(sp, valid, descs, pose, cur, cam=CAM, nnr=0.9, rng=None):
    n = len(sp)
    rng = rng or np.random.default_rng(n + 1)
    skip = np.asarray(valid) == 0
    bad = skip & (rng.random(n) < 0.5)
    return {"params": np.array([nnr], f64), "pose": np.asarray(pose, f32), "cam": HM.cam10(cam), "ml_sp": np.asarray(sp, f32).reshape(n, 3),
            "ml_ep": (np.asarray(sp, f32).reshape(n, 3) + f32(0.5)).astype(f32), "ml_bad": bad.astype(np.uint8),
            "ml_seen": (skip & ~bad).astype(np.uint8), "ml_desc": np.asarray(descs, np.uint8).reshape(n, 32),
            "cur_desc": np.asarray(cur, np.uint8).reshape(-1, 32)}


class LinesCase(Case):
    """Tracking.cc:3862-3877 on one frame; the match of :3882 stays with the stereo pin's matchNNR."""
    fn = "frustum_lines"

    def bag(self, a):
        bag = {"fn": _fn(self.fn), "params": a["params"]}
        bag.update(_frame_bag(a))
        bag.update({k: a[k] for k in ("ml_sp", "ml_ep", "ml_bad", "ml_seen")})
        return bag

    def valid(self, a):
        return ((a["ml_bad"] == 0) & (a["ml_seen"] == 0)).astype(np.uint8)

    def expected(self, a, res):
        return res["in_view"], res["proj_s"], res["list"], int(res["n_to_match"][0])

    def restate(self, a, misread=(), exits=None):
        in_view, proj = lm.is_in_frustum_l(a["ml_sp"], self.valid(a), a["pose"], HM.cam_of(a["cam"]), exits=exits, misread=misread)
        lst = np.flatnonzero(in_view).astype(np.int32)
        return in_view, proj, lst, len(lst)

    def device(self, fe, a):
        """-> the four pinned answers, and the match with the restatement's answer for the pinned list beside it."""
        in_view, proj, lst, m, n = fe.search_local_lines(a["ml_sp"], self.valid(a), a["ml_desc"], a["pose"], HM.cam_of(a["cam"]), a["cur_desc"],
                                                         float(a["params"][0]))
        return (in_view, proj, lst, len(lst)), (m, n)

    @staticmethod
    def same(want, got):
        return (np.asarray(want[0], np.int32).tobytes() == np.asarray(got[0], np.int32).tobytes() and lm.canonical(want[1]) == lm.canonical(got[1])
                and np.asarray(want[2], np.int32).tobytes() == np.asarray(got[2], np.int32).tobytes() and int(want[3]) == int(got[3]))


def _scene_lines(nl, none=False):
    def make():
        pose, sp, valid, descs, cur = lm.line_scene(SEED, 300, 60)
        valid = np.zeros(nl, np.uint8) if none else valid[:nl]
        return lines_arrays(sp[:nl], valid, descs[:nl], pose, cur)
    return make


def _constructed_lines():
    sp = np.concatenate([points_on_the_bounds(divide=False, seed=6), lm.line_where_the_two_forms_disagree(),
                         np.array([[0.1, 0.1, -1e-6], [0.0, 0.0, 0.0], [1.0, 0.0, 0.0]], f32)])
    rng = np.random.default_rng(8)
    return lines_arrays(sp, np.ones(len(sp), np.uint8), rng.integers(0, 256, (len(sp), 32), dtype=np.uint8), lm.IDENTITY,
                        rng.integers(0, 256, (5, 32), dtype=np.uint8))


LINE_SIZES = (0, 1, 64, 65, 300)


# ================================================================================================ ComputeDistinctiveDescriptors
def groups_of(a):
    """Per feature the (N, 32) rows of vDescriptors: its observations by ascending keyframe (the pointer order of mObservations),
    bad keyframes left out; None for a feature that returns before it looks (mbBad)."""
    nf = len(a["ft_bad"])
    per = [[] for _ in range(nf)]
    for f, k, r in a["obs"]:
        per[f].append((int(k), int(r)))
    out = []
    for f in range(nf):
        if a["ft_bad"][f]:
            out.append(None)
            continue
        rows = [a["kf_desc"][k, r] for k, r in sorted(dict(per[f]).items()) if not a["kf_bad"][k]]
        out.append(np.array(rows, np.uint8).reshape(-1, 32))
    return out


def distinctive_arrays(groups, lines, bad_features=(), bad_kfs=(), seed=0):
    """Feature f observes keyframes drawn in ascending order, one row each; a bad keyframe is put INSIDE the groups it joins (its
    row is a decoy that would win: all its bits equal the group's first row), and the obs are listed in shuffled order."""
    rng = np.random.default_rng(seed)
    nf = len(groups)
    nkf = max([len(g) for g in groups] + [1]) + len(bad_kfs) + 3
    live = [k for k in range(nkf) if k not in bad_kfs]
    kf_desc = np.zeros((nkf, max(nf, 1), 32), np.uint8)
    obs = []
    for f, g in enumerate(groups):
        ks = sorted(rng.choice(live, len(g), replace=False).tolist()) if len(g) else []
        for k, row in zip(ks, g):
            kf_desc[k, f] = row
            obs.append((f, k, f))
        if len(g) > 1:
            for k in bad_kfs:
                kf_desc[k, f] = g[0]
                obs.append((f, k, f))
    obs = np.array(obs, np.int32).reshape(-1, 3)
    obs = obs[rng.permutation(len(obs))]
    kf_bad = np.zeros(nkf, np.uint8)
    kf_bad[list(bad_kfs)] = 1
    ft_bad = np.zeros(nf, np.uint8)
    ft_bad[list(bad_features)] = 1
    return {"params": np.array([lines], f64), "kf_desc": kf_desc, "kf_bad": kf_bad, "ft_bad": ft_bad, "obs": obs}


class DistinctiveCase(Case):
    fn = "distinctive"

    def __init__(self, name, arrays, tags=(), distinct=True):
        Case.__init__(self, name, arrays, tags)
        self.distinct = distinct                                          # every group's rows differ: the row names BestIdx

    def bag(self, a):
        bag = {"fn": _fn(self.fn)}
        bag.update(a)
        return bag

    def lines(self, a):
        return bool(a["params"][0])

    def expected(self, a, res):
        """-> per feature BestIdx (-1: mDescriptor not written) where rows are distinct, and the descriptor bytes"""
        return (res["row"] if self.distinct else None), res["written"], res["desc"]

    def answer(self, a, best):
        """What a yardstick's or the device's BestIdx per feature (-1 / None: no answer) makes of the case."""
        groups = groups_of(a)
        nf = len(groups)
        row, written, desc = np.full(nf, -1, np.int32), np.zeros(nf, np.uint8), np.zeros((nf, 32), np.uint8)
        for f, g in enumerate(groups):
            if g is None or len(g) == 0:
                continue
            row[f], written[f], desc[f] = best[f], 1, g[best[f]]
        return (row if self.distinct else None), written, desc

    def restate(self, a, fn=None, mut=()):
        fn = fn or (HD.restated_line if self.lines(a) else HD.restated_point)
        kw = {"mut": mut} if mut else {}
        return self.answer(a, [None if g is None or len(g) == 0 else fn(g, **kw)[0] for g in groups_of(a)])

    def device(self, fe, a):
        groups = [np.zeros((0, 32), np.uint8) if g is None else g for g in groups_of(a)]
        best, _, _ = fe.distinctive_descriptors(groups)
        return self.answer(a, best)

    @staticmethod
    def same(want, got):
        return ((want[0] is None or np.array_equal(want[0], got[0])) and np.array_equal(want[1], got[1]) and np.array_equal(want[2], got[2]))


def _distinct_track(rng, n, flip):
    while True:
        g = HD.track(rng, n, flip)
        if len({r.tobytes() for r in g}) == n:
            return g


def _sized_groups(lines, seed):
    def make():
        rng = np.random.default_rng(seed)
        groups = [_distinct_track(rng, n, float(rng.choice([0.05, 0.15, 0.5]))) for n in (1, 2, 3, 4, 64, 65, 257, 5, 0, 12, 7)]
        return distinctive_arrays(groups, lines, bad_features=(7,), bad_kfs=(3, 40), seed=seed)
    return make


def _hand_groups(lines, distinct):
    def make():
        hg = HD.hand_groups()
        names = [n for n in sorted(hg) if (len({r.tobytes() for r in hg[n][0]}) == len(hg[n][0])) == distinct]
        groups = [hg[n][0] for n in names]
        if not distinct:
            groups += [HD.complement_pairs(64), HD.complement_pairs(65)]
        else:                                                            # more ties for the least median: small tracks that have one
            rng = np.random.default_rng(31)
            while len(groups) < 24:
                g = _distinct_track(rng, int(rng.integers(3, 12)), 0.05)
                b, m, med = HD.restated_point(g)
                if med.count(m) > 1:
                    groups.append(g)
        return distinctive_arrays(groups, lines, seed=3)
    return make


# ============================================================================================== LocalMapping::CreateNewMapPoints
ULP1 = float(np.spacing(f32(0.5)))                                       # one float ulp below 1, where the parallax cosines lie


def new_points_arrays(kf1, nbrs, cam=NP.CAM, mb=NP.MB, mono=False, coarse=False, far=False, th_far=0.0, bf2=None):
    """The driver's tables of a helpers_new_map_points scene; F12 and the epipole are not inputs: the reference forms them from the
    poses (NewPointsCase.scene restates that with helpers_match_ref.tri_geometry).  bf2: an mbf of its own per neighbour."""
    from test_triangulation_search_cpu import SCALE as SF_TRI, SIGMA2 as SIGMA2_TRI
    a = {"params": np.array([mono, coarse, far, th_far], f64), "cam": np.array(list(cam) + [mb], f32), "scale": np.array([1.2], f32),
         "sf": np.asarray(SF_TRI, f32), "sigma2": np.asarray(SIGMA2_TRI, f32)}
    for k, kf in enumerate([kf1] + [nb.kf for nb in nbrs]):
        t, pre = kf.t, "k%d_" % k
        a.update({pre + "x": t.x.astype(f32), pre + "y": t.y.astype(f32), pre + "octave": t.octave.astype(np.int32), pre + "angle": t.angle.astype(f32),
                  pre + "desc": np.asarray(t.desc, np.uint8), pre + "node": t.node.astype(np.int32), pre + "has_mp": t.has_mp.astype(np.uint8),
                  pre + "uright": kf.uright.astype(f32), pre + "depth": kf.depth.astype(f32), pre + "key": kf.key.astype(f32),
                  pre + "pose": kf.pose.astype(f32)})
        if bf2 is not None and k > 0:
            a[pre + "bf"] = np.array([bf2[k - 1]], f32)
    return a


class NewPointsCase(Case):
    """One whole LocalMapping::CreateNewMapPoints() on a keyframe and its neighbours, one pinhole camera."""
    fn = "new_map_points"

    def bag(self, a):
        bag = {"fn": _fn(self.fn)}
        bag.update(a)
        return bag

    def scene(self, a):
        """-> kf1, nbrs (helpers_new_map_points.KF / NB) with the F12 and the epipole the reference forms, cam, mb, bf2, settings."""
        from test_triangulation_search_cpu import Table
        nkf = 0
        while "k%d_x" % (nkf + 1) in a:
            nkf += 1
        cam, mb = tuple(f32(v) for v in a["cam"][:5]), f32(a["cam"][5])
        K = a["cam"][:4]
        kfs = []
        for k in range(nkf + 1):
            g = lambda f: a["k%d_%s" % (k, f)]
            t = Table(g("x"), g("y"), g("octave"), g("angle"), g("desc"), g("node"), g("has_mp"), (g("uright") >= 0).astype(np.uint8))
            kfs.append(NP.KF(t, g("uright"), g("depth"), g("key"), g("pose")))
        p1 = kfs[0].pose
        nbrs = []
        for kf in kfs[1:]:
            F12, ep = HM.tri_geometry(p1[:9], p1[9:12], p1[12:15], K, kf.pose[:9], kf.pose[9:12], K)
            nbrs.append(NP.NB(kf, F12, ep, None))
        bf2 = [f32(a["k%d_bf" % k][0]) for k in range(1, nkf + 1)] if "k1_bf" in a else None
        mono, coarse, far, th_far = a["params"]
        return kfs[0], nbrs, cam, mb, bf2, dict(coarse=bool(coarse), far=bool(far), th_far=float(th_far))

    def expected(self, a, res):
        """-> matches12[nkf, n1] as the loop saw them, created[nkf, n1], x3d[nkf, n1, 3] (zero where nothing was created), and the
        creation sequence as rows (neighbour, idx1, idx2)."""
        kf1, nbrs = self.scene(a)[:2]
        nkf, n1 = len(nbrs), len(kf1.t.node)
        m, made, x = np.full((nkf, n1), -1, np.int32), np.zeros((nkf, n1), bool), np.zeros((nkf, n1, 3), f32)
        for k, i, j in res["pairs"]:
            m[k, i] = j
        for (k, i, j), p in zip(res["created"], res["x3d"]):
            assert m[k, i] == j                                            # a created point comes from a matched pair
            made[k, i], x[k, i] = True, p
        return m, made, x, res["created"]

    def _answer(self, out, order=None):
        m, n, st, x, nnew = out
        made = st == NP.CREATED
        x = np.where(made[..., None], x, f32(0)).astype(f32)
        if order is None:                                                  # neighbours in order, idx1 ascending, status == CREATED
            order = [(k, i, m[k, i]) for k in range(len(m)) for i in np.flatnonzero(made[k])]
        return m, made, x, np.array(order, np.int32).reshape(-1, 3)

    def restate(self, a, mut=(), closed=False, exits=None):
        kf1, nbrs, cam, mb, bf2, kw = self.scene(a)
        if closed:
            return self._answer(NP.closed_form(kf1, nbrs, cam=cam, mb=mb, mut=mut, bf2=bf2, **kw))
        order = []
        out = NP.create_new_map_points(kf1, nbrs, cam=cam, mb=mb, mut=tuple(m for m in mut if m != "last_wins"), bf2=bf2, order=order,
                                       exits=exits, **kw)
        return self._answer(out, [(k, i, j) for k, i, j, _ in order])

    def device(self, fe, a, chained=False):
        """All neighbours in one call, or one call per neighbour chained through has_mp by hand."""
        kf1, nbrs, cam, mb, bf2, kw = self.scene(a)
        camera = tuple(float(v) for v in cam) + (0.0, 752.0, 0.0, 480.0)
        kp = lambda t: HM.keypoints(t.x, t.y, t.octave, t.angle)
        kf_of = lambda kf, has: (kp(kf.t), kf.t.desc, kf.t.node, has, kf.uright, kf.depth, kf.key, kf.pose)
        call = lambda has1, nb: fe.create_new_map_points(kf_of(kf1, has1), [kf_of(n.kf, n.kf.t.has_mp) + (n.F12, n.ep) for n in nb], camera,
                                                         float(mb), float(NP.RATIO_FACTOR), kw["coarse"], kw["far"], kw["th_far"])
        if not chained:
            return self._answer(call(kf1.t.has_mp, nbrs))
        has1 = kf1.t.has_mp.copy()
        parts = []
        for nb in nbrs:
            parts.append(call(has1.copy(), [nb]))
            has1[parts[-1][2][0] == NP.CREATED] = 1
        n1 = len(has1)
        cat = lambda i, shape, dt: np.concatenate([p[i] for p in parts]) if parts else np.zeros(shape, dt)
        return self._answer((cat(0, (0, n1), np.int32), cat(1, (0,), np.int32), cat(2, (0, n1), np.int32), cat(3, (0, n1, 3), f32), cat(4, (0,), np.int32)))

    def judge(self, a, res):
        """What the generator adds under "f64": per rejected pair of vMatchedIndices the exit helpers_new_map_points.pair_f64 assigns,
        and the least distance, in float ulps below 1, of any parallax comparison of a pair with a stereo side from its threshold
        (cos(2 atan2(mb / 2, depth)) is the one quantity of the gates that a libm computes)."""
        kf1, nbrs, cam, mb, bf2, kw = self.scene(a)
        made = {(k, i) for k, i, j in res["created"]}
        exits, margin = [], math.inf
        for k, i, j in res["pairs"]:
            S1, S2 = NP.side(kf1, i), NP.side(nbrs[k].kf, j)
            name, _, margins, _ = NP.pair_f64(S1, S2, cam, mb, kw["far"], kw["th_far"])
            if S1["ur"] >= 0 or S2["ur"] >= 0:
                margin = min(margin, margins.get("cos", math.inf) / ULP1)
            if (k, i) not in made:
                exits.append(NP.CODE[name])
        return {"rejected_exit": np.array(exits, np.int32), "libm_margin_ulps": np.array([margin], f64)}

    @staticmethod
    def same(want, got):
        return (np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1]) and want[2].tobytes() == np.asarray(got[2], f32).tobytes()
                and np.array_equal(np.asarray(want[3]).reshape(-1, 3), np.asarray(got[3]).reshape(-1, 3)))


def _new_points_scene(seed, nkf, npts, stereo="mixed", mono=False, coarse=False, far=False, th_far=9.0, half_bf=False, on_a_dist=False):
    def make():
        kf1, nbrs = NP.scene(seed, nkf, npts, stereo=stereo)
        bf2 = [f32(0.5) * NP.CAM[4]] * nkf if half_bf else None
        a = new_points_arrays(kf1, nbrs, mono=mono, coarse=coarse, far=far, th_far=th_far, bf2=bf2)
        if on_a_dist:                            # mThFarPoints exactly on the larger distance of a pair the gate would let through
            c = NewPointsCase("", a)
            k1, nb, cam, mb, _, kw = c.scene(a)
            m, _, st, _, _ = NP.create_new_map_points(k1, nb, cam=cam, mb=mb, coarse=coarse, far=False)
            k, i = np.argwhere(st == NP.CREATED)[len(np.argwhere(st == NP.CREATED)) // 2]
            q = {}
            NP.new_map_point_pair(NP.side(k1, i), NP.side(nb[k].kf, int(m[k, i])), cam, mb, q=q)
            a["params"] = np.array([mono, coarse, True, max(q["dist1"], q["dist2"])], f64)
        return a
    return make


def _new_points_constructed(which):
    def make():
        c = [c for c in NP.constructed_scenes() if c["name"] == which][0]
        return new_points_arrays(c["kf1"], c["nbrs"], cam=c["cam"], mb=c["mb"])
    return make


# -------------------------------------------------------------------------------------- the mpCamera2 branch (:463-528)
def _po():
    from oracle import pyoracle
    pyoracle.lib()
    return pyoracle


def new_points_two_cameras_arrays(kf1, nbrs, coarse=False, far=False, th_far=0.0):
    """The driver's tables of a helpers_new_map_points_two_cameras scene: per keyframe the table (mvKeys, then mvKeysRight), NLeft
    and the LEFT pose; the right poses, the four relative poses and the epipole are not inputs (the reference forms them from the
    left pose and mTlr; TwoCamerasCase.scene restates that with test_triangulation_two_cameras_cpu's Pose)."""
    import helpers_new_map_points_two_cameras as N2
    import test_triangulation_two_cameras_cpu as T2
    a = {"params": np.array([0, coarse, far, th_far], f64), "cam": np.zeros(6, f32), "scale": np.array([1.2], f32), "sf": N2.SCALE32,
         "sigma2": N2.SIGMA32, "kb1": np.asarray(T2.CAMS[0], f32), "kb2": np.asarray(T2.CAMS[1], f32),
         "Tlr": np.hstack([T2.TLR_R, T2.TLR_T.reshape(3, 1)]).astype(f32)}
    for k, kf in enumerate([kf1] + [nb.kf for nb in nbrs]):
        t, pre = kf.t, "k%d_" % k
        a.update({pre + "x": t.x.astype(f32), pre + "y": t.y.astype(f32), pre + "octave": t.octave.astype(np.int32), pre + "angle": t.angle.astype(f32),
                  pre + "desc": np.asarray(t.desc, np.uint8), pre + "node": t.node.astype(np.int32), pre + "has_mp": t.has_mp.astype(np.uint8),
                  pre + "nleft": np.array([t.nleft], np.int32), pre + "pose": kf.pose[0].astype(f32)})
    return a


class TwoCamerasCase(NewPointsCase):
    """One whole CreateNewMapPoints() on keyframes of two KannalaBrandt8 cameras."""
    group = "new_map_points_two_cameras"

    def scene(self, a):
        """-> kf1, nbrs (helpers_new_map_points_two_cameras.KF / NB: both poses of every keyframe, the four relative poses and the
        epipole as the reference's getters and ORBmatcher.cc:995-1003 form them), settings."""
        import helpers_new_map_points_two_cameras as N2
        import test_triangulation_two_cameras_cpu as T2
        if getattr(self, "_scene", None) is None or self._scene[0] is not a:
            nkf = 0
            while "k%d_x" % (nkf + 1) in a:
                nkf += 1
            kfs, poses = [], []
            for k in range(nkf + 1):
                g = lambda f: a["k%d_%s" % (k, f)]
                t = T2.Table(g("x"), g("y"), g("octave"), g("angle"), g("desc"), g("node"), g("has_mp"), int(g("nleft")[0]))
                poses.append(T2.Pose(g("pose")[:9], g("pose")[9:12]))
                kfs.append(N2.KF(t, N2.pose30(poses[-1])))
                assert kfs[-1].pose[0].tobytes() == g("pose").tobytes()            # the stored Ow is the getter's
            nbrs = [N2.NB(kf, T2.relative_poses(poses[0], p), T2.epipole(poses[0], p)) for kf, p in zip(kfs[1:], poses[1:])]
            _, coarse, far, th_far = a["params"]
            self._scene = (a, kfs[0], nbrs, dict(coarse=bool(coarse), far=bool(far), th_far=float(th_far)))
        return self._scene[1:]

    def expected(self, a, res):
        kf1, nbrs, _ = self.scene(a)
        nkf, n1 = len(nbrs), len(kf1.t.node)
        m, made, x = np.full((nkf, n1), -1, np.int32), np.zeros((nkf, n1), bool), np.zeros((nkf, n1, 3), f32)
        for k, i, j in res["pairs"]:
            m[k, i] = j
        for (k, i, j), p in zip(res["created"], res["x3d"]):
            assert m[k, i] == j
            made[k, i], x[k, i] = True, p
        return m, made, x, res["created"]

    def restate(self, a, mut=(), closed=False, exits=None):
        import helpers_new_map_points_two_cameras as N2
        kf1, nbrs, kw = self.scene(a)
        rules = tuple(mut)
        if closed:
            return self._answer(N2.closed_form(_po(), kf1, nbrs, rules=rules, **kw))
        order = []
        out = N2.create_new_map_points(_po(), kf1, nbrs, rules=rules, order=order, exits=exits, **kw)
        return self._answer(out, [(k, i, j) for k, i, j, _ in order])

    def device(self, fe, a, chained=False):
        import helpers_new_map_points_two_cameras as N2
        import test_triangulation_two_cameras_cpu as T2
        kf1, nbrs, kw = self.scene(a)
        kp = lambda t: HM.keypoints(t.x, t.y, t.octave, t.angle)
        kf_of = lambda kf, has: (kp(kf.t), kf.t.desc, kf.t.node, has, kf.t.nleft, kf.pose)
        call = lambda has1, nb: fe.create_new_map_points_two_cameras(kf_of(kf1, has1), [kf_of(n.kf, n.kf.t.has_mp) + (n.rel,) for n in nb],
                                                                     T2.CAMS[0], T2.CAMS[1], N2.RATIO_FACTOR, kw["coarse"], kw["far"], kw["th_far"])
        if not chained:
            return self._answer(call(kf1.t.has_mp, nbrs))
        has1 = kf1.t.has_mp.copy()
        parts = []
        for nb in nbrs:
            parts.append(call(has1.copy(), [nb]))
            has1[parts[-1][2][0] == NP.CREATED] = 1
        return self._answer(tuple(np.concatenate([p[i] for p in parts]) for i in range(5)))

    def judge(self, a, res):
        """Under "f64": per rejected pair the exit helpers_new_map_points_two_cameras.pair_f64 assigns, and the least distance of a
        comparison that hangs on a libm (the KannalaBrandt8 unprojection in the parallax cosine, the projection in the two
        chi-square gates) from its threshold, in float ulps of the compared quantity, judged by that float64 statement."""
        import helpers_new_map_points_two_cameras as N2
        kf1, nbrs, kw = self.scene(a)
        made = {(k, i) for k, i, j in res["created"]}
        exits, margin = [], math.inf
        for k, i, j in res["pairs"]:
            S1, S2 = N2.side(kf1, i), N2.side(nbrs[k].kf, j)
            name, _, margins, q = N2.pair_f64(S1, S2, kw["far"], kw["th_far"])
            margin = min(margin, margins.get("cos", math.inf) / ULP1)
            for tag, S in (("e1", S1), ("e2", S2)):
                if tag in q:
                    g2 = 5.991 * float(N2.SIGMA32[S["octave"]])
                    margin = min(margin, abs(q[tag] ** 2 - g2) / float(np.spacing(f32(g2))))
            if (k, i) not in made:
                exits.append(NP.CODE[name])
        return {"rejected_exit": np.array(exits, np.int32), "libm_margin_ulps": np.array([margin], f64)}


    @staticmethod
    def same(want, got):
        """The decisions exactly (vMatchedIndices, which pairs became points, the creation sequence); x3D to the bound the helper of
        today's tests records for it, MEASURED["x3d_rel"] relative to the point's norm: xn = pCamera->unprojectMat(kp.pt) goes through
        KannalaBrandt8::unproject, whose atan / Newton steps are the C library's in the reference's build, and about one pixel in
        thirty unprojects one float away from the oracle's and the device's (tests/test_ref_pin_match_two_cameras.py explains each
        such float by one libm result); x3D follows by a few ulps.  The gates keep their answers: judge() holds every pair at least
        2 float ulps from them."""
        import helpers_new_map_points_two_cameras as N2
        if not (np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1])
                and np.array_equal(np.asarray(want[3]).reshape(-1, 3), np.asarray(got[3]).reshape(-1, 3))):
            return False
        w, g = want[2][want[1]].astype(f64), np.asarray(got[2], f32)[want[1]].astype(f64)
        return bool(len(w) == 0 or (np.linalg.norm(w - g, axis=1) <= N2.MEASURED["x3d_rel"] * np.linalg.norm(w, axis=1)).all())

    @staticmethod
    def bit_equal(want, got):
        """-> how many created points have the reference's x3D bit for bit, of how many"""
        made = want[1]
        return int((want[2][made].view(np.uint32) == np.asarray(got[2], f32)[made].view(np.uint32)).all(-1).sum()), int(made.sum())


def _two_cameras_scene(seed, nkf, npoints, coarse=False, far=False):
    def make():
        import helpers_new_map_points_two_cameras as N2
        kf1, nbrs, _ = N2.scene(seed, nkf, npoints)
        return new_points_two_cameras_arrays(kf1, nbrs, coarse=coarse, far=far, th_far=N2.TH_FAR)
    return make


TWO_CAMERAS_CASES = [TwoCamerasCase("newpts2_nkf1", _two_cameras_scene(5, 1, 150, coarse=True)),
                     TwoCamerasCase("newpts2_nkf3_far", _two_cameras_scene(6, 3, 262, far=True))]

NEW_POINT_CASES = [
    NewPointsCase("newpts_nkf1_mixed", _new_points_scene(11, 1, 300), tags=("mixed",)),
    NewPointsCase("newpts_nkf5_mixed_coarse_far", _new_points_scene(15, 5, 300, coarse=True, far=True, half_bf=True), tags=("mixed", "bf")),
    NewPointsCase("newpts_nkf3_far_on_a_dist", _new_points_scene(21, 3, 120, on_a_dist=True), tags=("far_eq",)),
    NewPointsCase("newpts_nkf2_mono", _new_points_scene(32, 2, 150, stereo="mono", mono=True), tags=("mono",)),
    NewPointsCase("newpts_nkf2_stereo", _new_points_scene(11, 2, 150, stereo="stereo", half_bf=True), tags=("stereo", "bf")),
    # (constructed_scenes' dist_zero needs an F12 of its own; the reference forms F12 from the poses and then matches nothing there)
    NewPointsCase("newpts_w_zero", _new_points_constructed("w_zero")),
]

# ========================================================================================================================= corpus
CASES = (
    [PointsCase("points_nq%d" % n, _scene_points(n, th, far)) for n, th, far in POINT_SIZES]
    + [PointsCase("points_stored_views", _scene_points(257, 3.0, False, stored=True), tags=("stored",)),
       PointsCase("points_stored_views_far", _scene_points(65, 1.0, True, stored=True), tags=("stored",)),
       PointsCase("points_constructed", _constructed_points, tags=("bounds", "nan", "view_cos", "dist_bounds")),
       PointsCase("points_infinite_ratio", _infinite_ratio), PointsCase("points_level_bounds", _level_bounds, tags=("level",))]
    + [LinesCase("lines_nl%d" % n, _scene_lines(n)) for n in LINE_SIZES]
    + [LinesCase("lines_none_in_view", _scene_lines(65, none=True)), LinesCase("lines_constructed", _constructed_lines, tags=("bounds",))]
    + [DistinctiveCase("distinctive_points_sizes", _sized_groups(0, 41)), DistinctiveCase("distinctive_lines_sizes", _sized_groups(1, 42)),
       DistinctiveCase("distinctive_points_hand", _hand_groups(0, True), tags=("tie",)),
       DistinctiveCase("distinctive_lines_hand", _hand_groups(1, True), tags=("tie",)),
       DistinctiveCase("distinctive_points_duplicates", _hand_groups(0, False), distinct=False),
       DistinctiveCase("distinctive_lines_duplicates", _hand_groups(1, False), distinct=False)]
    + NEW_POINT_CASES + TWO_CAMERAS_CASES
)
BY_NAME = {c.name: c for c in CASES}
BY_NAME["points_infinite_ratio"].undefined_level = (0,)
FUNCTIONS = ("frustum_points", "frustum_lines", "distinctive", "new_map_points", "new_map_points_two_cameras")
BY_FN = {fn: [c for c in CASES if (c.group or c.fn) == fn] for fn in FUNCTIONS}


def exit_counts():
    """Per function the exits the restatement takes over the fixtures' inputs (tools/gen_map_ref.py prints them, DESIGN.md §2 records them)."""
    out = {"frustum_points": Counter(), "frustum_lines": Counter()}
    for c in BY_FN["frustum_points"] + BY_FN["frustum_lines"]:
        c.restate(load_fixture(c.name)[0], exits=out[c.fn])
    return out
