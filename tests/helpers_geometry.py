"""An independent float64 restatement of the two stages that do camera geometry in floating point, CPU only, plain numpy.

  * track_expect     the projection half of ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono, match12)
                     (ORBmatcher.cc:2190-2244) with Frame::UnprojectStereo (Frame.cc:1334-1350) and mOw / mRwc of
                     Frame::UpdatePoseMatrices standing behind the last frame's map points;
  * fisheye_expect   KannalaBrandt8::TriangulateMatches / unproject / project / Triangulate (KannalaBrandt8.cpp:28-42,
                     103-130, 334-403, 422-435) for one left / right pair;
  * fisheye_frame    the loop of Frame::ComputeStereoFishEyeMatches over two tables (Frame.cc:1596-1617).

Written from the reference's text -- NOT from oracle/match_oracle.hpp and NOT from the kernels -- and shaped differently on
purpose, so that a misreading shared by the oracle and the kernels is not repeated here: poses are 4x4 homogeneous matrices and
every inverse is np.linalg.inv of one (no R.t(), no -R.t()*t written out); the triangulation is np.linalg.svd; the
unprojection iterates Newton to convergence in double (newton_steps = 10 restates the reference's ten float steps with its
1e-6 break, see below); the projection uses x / hypot and y / hypot instead of cos / sin of atan2; Lowe's ratio is decided in
integers (10 d0 < 7 d1, which is what `d0 < d1 * 0.7` in double decides for every pair of Hamming distances: `7 < 10 * 0.7`
is false).  The inputs are exactly the float32 values the device gets, widened to float64.

Every function reports, per case, the exit it took and the MARGIN of every gate it went through: the distance of the compared
quantity from its threshold, in the gate's own unit.  The corpus builders refuse a table in which a margin is below the
decided margin of that gate (TRACK_MARGIN / FISHEYE_MARGIN), so every committed case is decided in float32 as it is in float64
and no test needs an "undecided" bucket.  Cases whose float64 arithmetic is exact (identity rotations, power-of-two focal
length and depths: the known-answer tables) are marked `exact` and may sit ON a threshold; that is what they are for.
Refused tables: 0 for the committed seeds (the tests assert it and print it).

Measured, oracle (float32, the reference's operation order) against this file (float64), on the committed corpora, CPU.  The
constants below are these worsts rounded up; tests/test_independent_geometry.py measures them again on every run, prints them, and
fails when a run measures more than is recorded here.

  track    u, v, ur   worst 29.41 ulp of float32 (MEASURED_TRACK_ULP = 30), in pixels 6.99e-4 (MEASURED_TRACK_PX = 7.1e-4); radius
                      0 ulp (one product).  The ulp is taken at the magnitude of the value, and not below the principal-point
                      coordinate that is added last (a projection that lands on u = 0.01 still carries the rounding of cx).
                      Tolerance TRACK_TOL_ULP = 4 x worst = 120 ulp, 2e-3 px at 185 px -- a wrong formula is off by whole pixels.
                      Decided margin of the image gate: 8 x 7.1e-4 = 5.7e-3 px.  Probes and decoys of the constructed current
                      frames sit 2 x that (TRACK_PROBE_PX = 1.1e-2 px) inside / outside the radius and the uRight gate.
           x3Dc.z     is not an output of the oracle; its deviation is bounded, not measured: four roundings (x3Dc of the last
                      frame, mOw, x3Dw, x3Dc) of values below 128 m, each at most ulp(128) / 2 = 3.8e-6 m, mixed by rotations
                      (factor sqrt(3)): 2.7e-5 m.  The decided margin is far wider, because it is also the corpus's depth range:
                      0.3 - 40 m in the camera that looks at the point, the CURRENT one included (a point 3 cm in front of the
                      current camera projects with a relative error of ulp(coordinates) / 0.03 and would be the only thing the
                      figures above measure).  A depth that leaves the point within 0.3 m of the current camera's plane is drawn
                      again, row by row, as part of the draw; the exact tables are exempt (their x3Dc.z is one exact subtraction).
           tlc.z      same bound, 2.7e-5 m; decided margin 8 x that, rounded up: 2.5e-4 m (the exact tables sit ON +-mb and one
                      ulp either side: tlc.z is one exact subtraction there).
  fisheye  depth, p3d worst c in |diff| <= c 2^-23 max(1, z^2 / |t12|): 5.21 (MEASURED_FISHEYE_C["default"] = 6), tolerance 4 x = 24.
                      Keypoints towards the image corner (70 - 78 degrees off the axis) have a depth of a quarter of their range,
                      so the z-based unit is small for them: their table ("tumvi_corner") is measured on its own, 46.3 (recorded
                      47, tolerance 188).  Against the GENERATING points of the noise-free pairs: c = 4.0 with the unit taken at
                      the range (bound: the tolerance + 4 units for the rounding of the four pixel coordinates to float32).
           cosParallaxRays   from the oracle's own rays (orc_kb8_unproject) against the float64 rays, plus the final float
                      rounding 2^-24: 8.98e-8 (MEASURED_COS = 1e-7).  Decided margin 8 x = 8e-7.
           reprojection      the oracle's orc_kb8_project of the oracle's p3d against the float64 projection of the float64
                      point: 2.27e-4 px (MEASURED_REPROJ_PX = 2.5e-4); the chi-square gates are compared as sqrt(err^2) against
                      sqrt(5.991 sigma^2), in pixels.  Decided margin 8 x = 2e-3 px.
           z1, z2, depth floor   8 x the measured c, in the unit of the depth tolerance at the case's own depth.
  Newton   the reference's ten steps with its 1e-6 break against the converged root, as rays, on every keypoint that is
           unprojected: 8.3e-13 relative (MEASURED_NEWTON = 1e-12), five orders below the float rounding of the ray; no label
           changes with newton_steps = 10 (asserted).  The ten fixed steps are the reference's behaviour and stay what they are.
  z2       IS reachable: see RIGS["wide"] and RIGS["fold"].

`TrackRules` / `FisheyeRules` hold the readings that the mutation tests flip; the defaults are the reference's.
"""
import math
from dataclasses import dataclass, replace  # noqa: F401  (replace: for the tests)

import numpy as np

import helpers_matchers as hm
from helpers_matchers import KEYPOINT_DT, f32

EPS32 = 2.0 ** -23

# ---- measured on the CPU (see the docstring; tests/test_independent_geometry.py measures them again and prints them) ----
MEASURED_TRACK_ULP = 30.0
MEASURED_TRACK_PX = 7.1e-4
MEASURED_FISHEYE_C = {"default": 6.0, "corner": 47.0}
MEASURED_COS = 1.0e-7
MEASURED_REPROJ_PX = 2.5e-4
MEASURED_NEWTON = 1.0e-12
# ---- derived ----
TRACK_TOL_ULP = 4 * MEASURED_TRACK_ULP
TRACK_MARGIN = {"image_px": 8 * MEASURED_TRACK_PX, "zc_m": 0.3, "motion_m": 2.5e-4}
TRACK_PROBE_PX = 2 * TRACK_MARGIN["image_px"]
FISHEYE_TOL_C = {k: 4 * v for k, v in MEASURED_FISHEYE_C.items()}
FISHEYE_MARGIN = {"cos": 8 * MEASURED_COS, "px": 8 * MEASURED_REPROJ_PX, "z_c": {k: 8 * v for k, v in MEASURED_FISHEYE_C.items()}}


# ---------------------------------------------------------------------------------------------------------------------
# descriptors: rows of the 256 x 256 Sylvester-Hadamard matrix and their complements, 512 rows at Hamming distance 128 or 256
# from each other -- no distance between two different rows is anywhere near TH_HIGH = 100, ties and the rotation filter
# decide nothing
# ---------------------------------------------------------------------------------------------------------------------
def code_rows(n, first=0):
    assert first + n <= 512, (first, n)
    if n == 0:
        return np.zeros((0, 32), np.uint8)
    i = np.arange(first, first + n)
    j = np.arange(256)
    par = np.array([[bin(a & b).count("1") & 1 for b in j] for a in (i & 255)], np.uint8)
    par ^= (i >= 256).astype(np.uint8)[:, None]
    return np.packbits(par, axis=1)


def flip_bits(desc, k, rng):
    """desc with k different bits flipped."""
    out = desc.copy()
    for b in rng.choice(256, k, replace=False):
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def hom(T34):
    T = np.eye(4)
    T[:3] = np.asarray(T34, f32).reshape(3, 4).astype(np.float64)
    return T


# ---------------------------------------------------------------------------------------------------------------------
# SearchByProjection(CurrentFrame, LastFrame): the projection
# ---------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class TrackRules:
    forward_ge: bool = False                      # `tlc.z >= mb` instead of `>`
    swap_forward_backward_windows: bool = False   # bForward searches 0 .. octave, bBackward octave .. top
    radius_from_level_0: bool = False             # th * mvScaleFactors[0]
    ur_plus: bool = False                         # ur = u + mbf * invzc
    no_behind_gate: bool = False                  # `if(invzc<0) continue;` missing
    ow_sign: bool = False                         # mOw = +mRcw.t()*mtcw
    image_gate_strict: bool = False               # `u <= mnMinX || u >= mnMaxX`
    pose_of_previous_pair: bool = False           # frame f reads the pose rows of frames f-2, f-1 (track_pair)


TREF = TrackRules()


@dataclass(frozen=True)
class TrackCam:
    """pli_track_params as the device gets them (float32 values)."""
    fx: float
    fy: float
    cx: float
    cy: float
    bf: float
    th: float
    mono: bool
    min_x: float
    max_x: float
    min_y: float
    max_y: float

    def f(self, name):
        return float(f32(getattr(self, name)))

    @property
    def bounds(self):
        return (self.f("min_x"), self.f("max_x"), self.f("min_y"), self.f("max_y"))


def track_expect(last_kp, last_depth, Tlw, Tcw, params, scale_factors, rules=TREF):
    """-> dict: label (no_depth / behind / out_of_image / ok), u, v, ur, radius (float64; u, v, ur are computed for EVERY row,
    also where a gate stopped it: that is where a missing gate would look), lo, hi (level window, hi = -1: open), forward,
    backward, and the margins zc (m), image (px) per row and motion (m)."""
    p = params
    fx, fy, cx, cy, bf, th = (p.f(k) for k in ("fx", "fy", "cx", "cy", "bf", "th"))
    minx, maxx, miny, maxy = p.bounds
    mb = float(f32(bf) / f32(fx))                                   # Frame.cc:197, a float division
    Tl, Tc = hom(Tlw), hom(Tcw)
    Tlc = Tl @ np.linalg.inv(Tc)                                    # current camera -> last camera; its translation is tlc
    tz = Tlc[2, 3]
    forward = bool(tz >= mb if rules.forward_ge else tz > mb) and not p.mono
    backward = bool(-tz > mb) and not p.mono
    Twl = np.linalg.inv(Tl)                                         # last camera -> world: [mRwc | mOw]
    if rules.ow_sign:
        Twl[:3, 3] = -Twl[:3, 3]
    M = Tc @ Twl                                                    # last camera -> current camera
    n = len(last_kp)
    z = np.asarray(last_depth, f32).astype(np.float64)
    x0, y0 = last_kp["x"].astype(np.float64), last_kp["y"].astype(np.float64)
    octave = last_kp["octave"].astype(np.int64)
    with np.errstate(all="ignore"):
        Xl = np.stack([(x0 - cx) * z / fx, (y0 - cy) * z / fy, z, np.ones(n)])
        Xc = M @ Xl
        zc = Xc[2]
        u = fx * Xc[0] / zc + cx
        v = fy * Xc[1] / zc + cy
        ur = u + bf / zc if rules.ur_plus else u - bf / zc
        has_depth = z > 0
        behind = (1.0 / zc) < 0                                     # `invzc < 0`: false for zc == 0 (+inf) and for NaN
        if rules.image_gate_strict:
            outside = (u <= minx) | (u >= maxx) | (v <= miny) | (v >= maxy)
        else:
            outside = (u < minx) | (u > maxx) | (v < miny) | (v > maxy)
        image_margin = np.minimum(np.minimum(np.abs(u - minx), np.abs(u - maxx)), np.minimum(np.abs(v - miny), np.abs(v - maxy)))
    label = np.full(n, "ok", object)
    label[outside] = "out_of_image"
    if not rules.no_behind_gate:
        label[behind] = "behind"
    label[~has_depth] = "no_depth"
    sf = np.asarray(scale_factors, f32).astype(np.float64)
    radius = th * (sf[0] if rules.radius_from_level_0 else sf[octave])
    fw, bw = (backward, forward) if rules.swap_forward_backward_windows else (forward, backward)
    if fw:
        lo, hi = octave.copy(), np.full(n, -1, np.int64)
    elif bw:
        lo, hi = np.zeros(n, np.int64), octave.copy()
    else:
        lo, hi = octave - 1, octave + 1
    motion = np.inf if p.mono else min(abs(tz - mb), abs(-tz - mb))
    return {"label": label, "u": u, "v": v, "ur": ur, "radius": radius * np.ones(n), "lo": lo, "hi": hi, "forward": forward,
            "backward": backward, "zc": np.abs(zc), "image": image_margin, "motion": motion, "tlc_z": tz, "mb": mb}


def track_pair(batch, f, rules=TREF):
    """Frame f of a batch against frame f - 1: which pose rows belong to it is part of the statement."""
    poses = batch["poses"]
    l, c = (max(f - 2, 0), f - 1) if rules.pose_of_previous_pair else (f - 1, f)
    fr = batch["frames"][f - 1]
    return track_expect(fr["kp"], fr["depth"], poses[l], poses[c], batch["cam"], batch["sf"], rules)


def track_undecided(E, exact=False):
    """Rows of a pair that sit closer to a gate than the decided margin (exact tables: closer, but not ON it)."""
    with np.errstate(invalid="ignore"):
        lab = E["label"]
        thin_z = (lab != "no_depth") & (E["zc"] < TRACK_MARGIN["zc_m"])
        thin_i = ((lab == "ok") | (lab == "out_of_image")) & (E["image"] < TRACK_MARGIN["image_px"])
        if exact:
            thin_z[:] = False                                       # (x3Dc.z is one exact subtraction there)
            thin_i &= E["image"] != 0
    motion_thin = E["motion"] < TRACK_MARGIN["motion_m"] and not exact    # (exact tables: tlc.z is one exact subtraction)
    return int(thin_z.sum() + thin_i.sum() + (len(lab) if motion_thin else 0))


def queries_from(E, last_kp):
    """pli_proj_query records from an expectation (float32), for helpers_matchers.search_by_projection: valid only where the
    restatement's own gates let the row through, so that search's image gate decides nothing."""
    q = np.zeros(len(last_kp), hm.PROJ_QUERY_DT)
    with np.errstate(all="ignore"):
        ok = (E["label"] == "ok") & np.isfinite(E["u"]) & np.isfinite(E["v"])   # (a NaN projection: every comparison with it is false)
        for k in ("u", "v", "ur", "radius"):
            q[k] = np.where(ok, E[k], 0).astype(f32)
    q["min_level"], q["max_level"] = np.where(ok, E["lo"], 0), np.where(ok, E["hi"], -1)
    q["angle"] = last_kp["angle"]
    q["valid"] = ok
    return q


def _rot(rx, ry, rz):
    cx_, sx = math.cos(rx), math.sin(rx)
    cy_, sy = math.cos(ry), math.sin(ry)
    cz, sz = math.cos(rz), math.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx_, -sx], [0, sx, cx_]])
    Ry = np.array([[cy_, 0, sy], [0, 1, 0], [-sy, 0, cy_]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def pose34(R, centre):
    """mTcw (float32 3x4) of a camera with orientation R (world -> camera) whose centre is `centre`."""
    T = np.zeros((3, 4))
    T[:, :3] = R
    T[:, 3] = -R @ np.asarray(centre, np.float64)
    return T.astype(f32)


def moved(T34, rot_deg, step):
    """The pose after the camera turns by rot_deg (about its own x, y, z) and moves by `step` metres in its own old frame."""
    T = hom(T34)
    D = np.eye(4)
    D[:3, :3] = _rot(*np.deg2rad(rot_deg))
    D[:3, 3] = -D[:3, :3] @ np.asarray(step, np.float64)
    return (D @ T)[:3].astype(f32)


class _Rows:
    def __init__(self):
        self.x, self.y, self.o, self.ur, self.desc, self.role = [], [], [], [], [], []

    def add(self, x, y, o, ur, desc, role):
        self.x.append(x); self.y.append(y); self.o.append(o); self.ur.append(ur); self.desc.append(desc); self.role.append(role)
        return len(self.x) - 1


def _probes(E, last, cam, nlevels, rng, max_no_depth=12):
    """The current frame that makes every decision of E visible in best_idx2.  Per last keypoint j that gets through (ok): ONE row
    it must take -- its descriptor with two bits flipped, inside radius, level window and uRight gate by TRACK_PROBE_PX / at the
    window's edge -- and decoys with the IDENTICAL descriptor (distance 0 beats 2 whatever the visiting order is) that only a
    wrong reading admits: one level outside the window, TRACK_PROBE_PX outside the radius, uRight TRACK_PROBE_PX beyond the
    radius.  Per last keypoint that a gate stops (of those without depth: the first max_no_depth): the identical descriptor where a
    missing gate would look, at the keypoint's own level; where the projection is not finite, at the keypoint's own position.
    -> rows, expected (index into rows or -1 per last keypoint)."""
    minx, maxx, miny, maxy = cam.bounds
    m = TRACK_PROBE_PX
    last_kp, last_desc = last["kp"], last["desc"]
    R = _Rows()
    exp = np.full(len(E["label"]), -1, np.int64)
    top = nlevels - 1

    def inside(x, y):
        return minx + 0.5 <= x <= maxx - 0.5 and miny + 0.5 <= y <= maxy - 0.5

    n_no_depth = 0
    for j, lab in enumerate(E["label"]):
        u, v, ur, r = E["u"][j], E["v"][j], E["ur"][j], E["radius"][j]
        d = last_desc[j]
        own = int(last_kp["octave"][j])
        if lab == "no_depth":
            # (a decoy of the pair before shares its descriptor with the row it was a decoy for: it gets nothing here)
            if last["roles"][j][0] not in ("take", "query", "filler") or n_no_depth >= max_no_depth:
                continue
            n_no_depth += 1
        if not (np.isfinite(u) and np.isfinite(v) and np.isfinite(ur)):
            if lab != "no_depth":
                R.add(min(max(float(last_kp["x"][j]), minx + 1), maxx - 1), min(max(float(last_kp["y"][j]), miny + 1), maxy - 1), own,
                      -1.0, d, ("gate", j))
            continue
        if lab != "ok":
            # where a missing gate would look: the projection itself when it is a legal keypoint position, else the nearest
            # one if that is still inside the window
            x, y = min(max(u, minx + 1), maxx - 1), min(max(v, miny + 1), maxy - 1)
            if max(abs(x - u), abs(y - v)) < r - m:
                R.add(x, y, own, -1.0, d, ("gate", j))
            continue
        lo, hi = int(E["lo"][j]), int(E["hi"][j])
        hi_eff = top if hi < 0 else min(hi, top)
        lo_eff = max(lo, 0)
        # the row to take: at radius - m on one axis (the sign that stays inside the image), anywhere on the other
        sx = 1.0 if u + r < maxx - 1 else -1.0
        sy = 1.0 if v + r < maxy - 1 else -1.0
        if rng.random() < 0.5:
            dx, dy = sx * (r - m), sy * rng.uniform(0, 0.5) * r
        else:
            dx, dy = sx * rng.uniform(0, 0.5) * r, sy * (r - m)
        x, y = u + dx, v + dy
        if not inside(x, y):                                        # (windows wider than the image: stay next to the projection)
            x, y = min(max(u, minx + 1), maxx - 1), min(max(v, miny + 1), maxy - 1)
        level = lo_eff if rng.random() < 0.5 else hi_eff            # an edge of the window
        kind = rng.integers(3)
        good_ur = -1.0 if kind == 0 else ur + (r - m) * (1 if kind == 1 else -1)
        if good_ur <= 0:
            good_ur = -1.0
        exp[j] = R.add(x, y, level, good_ur, flip_bits(d, 2, rng), ("take", j))
        for lv in (lo - 1, hi + 1 if hi >= 0 else nlevels):        # one level outside (forward: octave - 1, backward: octave + 1)
            if 0 <= lv <= top:
                R.add(x, y, lv, -1.0, d, ("level", j))
        for ax in (0, 1):                                           # radius + m on one axis
            xx, yy = (u + sx * (r + m), y) if ax == 0 else (x, v + sy * (r + m))
            if inside(xx, yy):
                R.add(xx, yy, level, -1.0, d, ("radius", j))
        for sg in (1, -1):                                          # |ur - uright| = radius + m
            bad = ur + sg * (r + m)
            if bad > 0:
                R.add(x, y, level, bad, d, ("uright", j))
                break
    return R, exp


def _frame_from_rows(R, exp, n_rows, depth_of, rng, first_code):
    """Rows + fillers in a random order as a frame table: kp, desc, uright, depth; `exp` remapped to the new order."""
    n0 = len(R.x)
    assert n0 <= n_rows, (n0, n_rows)
    nfill = n_rows - n0
    fill_desc = code_rows(nfill, first_code) if nfill else np.zeros((0, 32), np.uint8)
    order = rng.permutation(n_rows)                                 # new position -> old row (>= n0: a filler)
    pos = np.empty(n_rows, np.int64)
    pos[order] = np.arange(n_rows)
    kp = np.zeros(n_rows, KEYPOINT_DT)
    desc = np.zeros((n_rows, 32), np.uint8)
    ur = np.full(n_rows, -1.0, f32)
    for new, old in enumerate(order):
        if old < n0:
            kp["x"][new], kp["y"][new], kp["octave"][new] = R.x[old], R.y[old], R.o[old]
            ur[new], desc[new] = R.ur[old], R.desc[old]
        else:
            kp["x"][new], kp["y"][new], kp["octave"][new] = rng.uniform(5, 370), rng.uniform(5, 235), rng.integers(0, 8)
            desc[new] = fill_desc[old - n0]
    kp["size"], kp["angle"] = 31.0, rng.uniform(0, 360, n_rows).astype(f32)
    roles = [R.role[old] if old < n0 else ("filler", -1) for old in order]
    depth = depth_of(roles, rng)
    return {"kp": kp, "desc": desc, "uright": ur, "depth": depth, "roles": roles}, np.where(exp >= 0, pos[np.maximum(exp, 0)], -1)


def _depths(roles, rng, lo=0.3, hi=40.0, active=60):
    """Depth per row as a last frame: rows that a query must take become the next queries (distinct descriptors), log-uniform in
    lo .. hi m; every other row has no depth: -1, 0 or NaN."""
    n = len(roles)
    depth = rng.choice(np.array([-1.0, 0.0, np.nan, -3.5], f32), n)
    cand = [i for i, r in enumerate(roles) if r[0] in ("take", "query")] or list(range(n))
    for i in rng.permutation(cand)[:active]:
        depth[i] = np.exp(rng.uniform(np.log(lo), np.log(hi)))
    return depth.astype(f32)


def _first_frame(n, rng, cam, depth_of):
    kp = np.zeros(n, KEYPOINT_DT)
    kp["x"], kp["y"] = rng.uniform(cam.f("min_x") + 2, cam.f("max_x") - 2, n), rng.uniform(cam.f("min_y") + 2, cam.f("max_y") - 2, n)
    kp["octave"] = rng.integers(0, 8, n)
    kp["octave"][:2] = (0, 7)[:min(n, 2)]                          # (both ends of the pyramid are always there)
    kp["size"], kp["angle"] = 31.0, rng.uniform(0, 360, n).astype(f32)
    roles = [("query", i) for i in range(n)]
    return {"kp": kp, "desc": code_rows(n), "uright": np.full(n, -1.0, f32), "depth": depth_of(roles, rng), "roles": roles}


def build_track_batch(name, cam, poses, sizes, seed, exact=False, first=None, depth_of=_depths, nlevels=8, scale=1.2):
    """A batch of len(poses) frames: frame 0 is `first` (or random), frame f the probe table of pair f.  -> batch dict with
    frames, poses, expected (per pair, index into frame f or -1) and `refused` (rows too close to a gate)."""
    rng = np.random.default_rng(seed)
    sf, _ = hm.scale_factors(nlevels, scale)
    batch = {"name": name, "cam": cam, "sf": sf, "poses": np.asarray(poses, f32).reshape(-1, 12), "exact": exact, "frames": [],
             "expected": [None], "E": [None], "refused": 0}
    batch["frames"].append(first if first is not None else _first_frame(sizes[0], rng, cam, depth_of))

    def settle(f):
        """The corpus's depths are 0.3 - 40 m in the camera that looks at the point, the current one included: a depth that leaves
        the point within TRACK_MARGIN["zc_m"] of the current camera's plane is drawn again (a rule of the draw, row by row)."""
        fr = batch["frames"][f]
        while not exact and f + 1 < len(batch["poses"]) and len(fr["kp"]):
            E = track_expect(fr["kp"], fr["depth"], batch["poses"][f], batch["poses"][f + 1], cam, sf)
            near = (E["label"] != "no_depth") & (E["zc"] < TRACK_MARGIN["zc_m"])
            if not near.any():
                break
            fr["depth"][near] = np.exp(rng.uniform(np.log(0.3), np.log(40.0), int(near.sum())))

    settle(0)
    for f in range(1, len(batch["poses"])):
        E = track_pair(batch, f)
        batch["refused"] += track_undecided(E, exact)
        R, exp = _probes(E, batch["frames"][f - 1], cam, nlevels, rng)
        n_rows = sizes[f] if sizes[f] is not None else len(R.x)
        frame, exp = _frame_from_rows(R, exp, n_rows, depth_of, rng, 256)
        batch["frames"].append(frame)
        settle(f)
        batch["expected"].append(exp)
        batch["E"].append(E)
    return batch


_TRACK = None


def track_corpus():
    """The committed track batches (built once per process)."""
    global _TRACK
    if _TRACK is not None:
        return _TRACK
    W, H = 376.0, 240.0
    cam = TrackCam(fx=435.2047, fy=431.7031, cx=185.3, cy=122.8, bf=47.90639, th=15.0, mono=False, min_x=0.0, max_x=W, min_y=0.0,
                   max_y=H)
    out = []
    # real rotations about all three axes, the world origin several metres away; the three pairs are neutral (a turn that
    # pushes a third of the projections out of the image), forward (2 m: a third of the points end up behind the camera) and
    # backward, each with its own rotation.  Last frames of 255 / 256 / 257 rows.
    p0 = pose34(_rot(0.35, -0.6, 0.17), (3.0, -2.0, 5.0))
    p1 = moved(p0, (1.5, -12.0, 2.0), (0.04, -0.02, 0.05))
    p2 = moved(p1, (-2.0, 3.0, -4.0), (0.1, 0.05, 2.0))
    p3 = moved(p2, (3.0, 2.5, 5.0), (-0.08, 0.03, -0.6))
    out.append(build_track_batch("stereo_three_motions", cam, [p0, p1, p2, p3], [255, 256, 257, None], seed=11))
    # the same motions seen by a monocular search: bMono leaves the neutral window even for |tlc.z| > mb
    camm = replace(cam, mono=True, th=7.0)
    out.append(build_track_batch("mono", camm, [p0, p2, p3], [90, 200, None], seed=12))
    # a pair whose last frame is empty, then a pair that is not
    out.append(build_track_batch("empty_last_frame", cam, [p0, p1, p2], [0, 40, None], seed=13,
                                 first=_first_frame(0, np.random.default_rng(0), cam, _depths)))
    out.extend(exact_track_batches())
    _TRACK = out
    return out


EXACT_CAM = TrackCam(fx=512.0, fy=512.0, cx=188.0, cy=120.0, bf=64.0, th=15.0, mono=False, min_x=0.0, max_x=376.0, min_y=0.0,
                     max_y=240.0)


def exact_first_frame(zero_rows):
    """Keypoints whose whole chain is exact in float32 and float64 for identity rotations and translations along z: integer
    pixel offsets from the principal point, power-of-two depths, fx = fy = 512."""
    xs = [188.0, 376.0, 100.0, 188.0, 376.0, 0.0, 250.0, 60.0, 188.0, 300.0]
    ys = [120.0, 120.0, 0.0, 0.0, 0.0, 240.0, 200.0, 30.0, 120.0, 50.0]
    zs = [2.0, 2.0, 4.0, 1.0, 8.0, 2.0, 0.5, 16.0, 0.125, 0.125]        # (the last two: x3Dc.z == 0 after a step of mb = 0.125)
    oc = [0, 7, 3, 1, 2, 5, 4, 6, 2, 3]
    if not zero_rows:
        xs, ys, zs, oc = xs[:8], ys[:8], zs[:8], oc[:8]
    n = len(xs)
    kp = np.zeros(n, KEYPOINT_DT)
    kp["x"], kp["y"], kp["octave"], kp["size"] = xs, ys, oc, 31.0
    return {"kp": kp, "desc": code_rows(n), "uright": np.full(n, -1.0, f32), "depth": np.array(zs, f32),
            "roles": [("query", i) for i in range(n)]}


def exact_track_batches():
    """Two-frame batches with Rlw = Rcw = I, tlw = 0 and tcw = (0, 0, -d): tlc.z == d exactly.  d = 0 (a keypoint projects onto
    itself; rows 1..5 land ON mnMaxX / mnMinY / mnMinX / mnMaxY), d = mb (strict: neutral; rows 8 and 9 have x3Dc.z == 0: u = NaN
    for row 8, whose x3Dc.x is 0 too, +inf for row 9), one ulp above (forward) and below (neutral), and the mirror for backward."""
    mb = f32(64.0) / f32(512.0)
    up, dn = np.nextafter(mb, f32(1)), np.nextafter(mb, f32(0))
    out = []
    for name, d in (("identity", f32(0)), ("tlc_eq_mb", mb), ("tlc_above_mb", up), ("tlc_below_mb", dn), ("tlc_eq_minus_mb", -mb),
                    ("tlc_below_minus_mb", -up), ("tlc_above_minus_mb", -dn)):
        T0 = np.eye(4)[:3].astype(f32)
        T1 = T0.copy()
        T1[2, 3] = -d
        out.append(build_track_batch("exact_" + name, EXACT_CAM, [T0, T1], [None, None], seed=21, exact=True,
                                     first=exact_first_frame(name in ("identity", "tlc_eq_mb"))))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# KannalaBrandt8 and ComputeStereoFishEyeMatches
# ---------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class FisheyeRules:
    r12_for_r21: bool = False             # Tcw2 built from R12 instead of R12.t()
    t21_sign: bool = False                # t21 = +R21*t12
    swap_sigmas: bool = False             # sigmaLevel from the right keypoint's octave, unc from the left one's
    ratio_le: bool = False                # `distance <= 0.7 * second`
    no_parallax_gate: bool = False
    no_z2_gate: bool = False
    first_left_keeps_right: bool = False  # mvRightToLeftMatch keeps the first left keypoint instead of the last


FREF = FisheyeRules()
HALF_PI_F = float(f32(math.pi / 2))       # fminf(..., CV_PI / 2.f)


def _cam(cam):
    return [float(f32(c)) for c in cam]


def kb8_unproject64(cam, u, v, newton_steps=None):
    """KannalaBrandt8::unproject: the ray (x, y, 1).  newton_steps = None: Newton on theta (1 + k0 theta^2 + ...) = theta_d until
    the step no longer changes theta; = 10: the reference's loop (ten steps at most, stop after a step below 1e-6)."""
    fx, fy, cx, cy, k0, k1, k2, k3 = _cam(cam)
    x, y = (float(u) - cx) / fx, (float(v) - cy) / fy
    td = min(math.hypot(x, y), HALF_PI_F)
    scale = 1.0
    if td > 1e-8:
        th = td
        for _ in range(100 if newton_steps is None else newton_steps):
            t2 = th * th
            fval = th * (1 + t2 * (k0 + t2 * (k1 + t2 * (k2 + t2 * k3)))) - td
            der = 1 + t2 * (3 * k0 + t2 * (5 * k1 + t2 * (7 * k2 + t2 * 9 * k3)))
            step = fval / der
            th -= step
            if abs(step) < (1e-15 if newton_steps is None else 1e-6):
                break
        scale = math.tan(th) / td
    return np.array([x * scale, y * scale, 1.0])


def kb8_project64(cam, P):
    fx, fy, cx, cy, k0, k1, k2, k3 = _cam(cam)
    rho = math.hypot(P[0], P[1])
    th = math.atan2(rho, P[2])
    t2 = th * th
    r = th * (1 + t2 * (k0 + t2 * (k1 + t2 * (k2 + t2 * k3))))
    cs, sn = (P[0] / rho, P[1] / rho) if rho > 0 else (1.0, 0.0)     # psi = atan2f(0, 0) = 0
    return np.array([fx * r * cs + cx, fy * r * sn + cy])


def rig_T21(R12, t12, rules=FREF):
    """Tcw2 of TriangulateMatches: camera 1 -> camera 2, the inverse of [R12 | t12]."""
    T12 = np.eye(4)
    T12[:3, :3] = np.asarray(R12, f32).reshape(3, 3).astype(np.float64)
    T12[:3, 3] = np.asarray(t12, f32).astype(np.float64)
    T21 = np.linalg.inv(T12)
    if rules.r12_for_r21:
        T21[:3, :3] = T12[:3, :3]
        T21[:3, 3] = -T12[:3, :3] @ T12[:3, 3]
    if rules.t21_sign:
        T21[:3, 3] = -T21[:3, 3]
    return T12, T21


def fisheye_expect(kp1, kp2, cam1, cam2, R12, t12, sigma2, d0=0, d1=256, rules=FREF, newton_steps=None):
    """One pair: kp = (x, y, octave) as the float32 the device gets.  -> label, margins {gate: distance}, X (camera 1) or None."""
    mg = {}
    if not (10 * d0 <= 7 * d1 if rules.ratio_le else 10 * d0 < 7 * d1):
        return "ratio", mg, None
    T12, T21 = rig_T21(R12, t12, rules)
    r1 = kb8_unproject64(cam1, kp1[0], kp1[1], newton_steps)
    r2 = kb8_unproject64(cam2, kp2[0], kp2[1], newton_steps)
    r21 = T12[:3, :3] @ r2
    cosp = float(r1 @ r21 / (np.linalg.norm(r1) * np.linalg.norm(r21)))
    mg["cos"], mg["_cos"] = abs(cosp - 0.9998), cosp
    if cosp > 0.9998 and not rules.no_parallax_gate:
        return "parallax", mg, None
    P1, P2 = np.eye(4)[:3], T21[:3]
    A = np.stack([r1[0] * P1[2] - P1[0], r1[1] * P1[2] - P1[1], r2[0] * P2[2] - P2[0], r2[1] * P2[2] - P2[1]])
    vt = np.linalg.svd(A)[2]
    X = vt[3, :3] / vt[3, 3]
    tn = float(np.linalg.norm(T12[:3, 3]))
    zscale = EPS32 * max(1.0, X[2] * X[2] / tn)                      # one unit of the depth tolerance at this depth
    mg["z1"] = abs(X[2]) / zscale
    if X[2] <= 0:
        return "z1", mg, None
    X2 = T21[:3] @ np.append(X, 1.0)
    mg["z2"] = abs(X2[2]) / zscale
    if X2[2] <= 0 and not rules.no_z2_gate:
        return "z2", mg, None
    s1, s2 = float(sigma2[int(kp1[2])]), float(sigma2[int(kp2[2])])
    if rules.swap_sigmas:
        s1, s2 = s2, s1
    e1 = kb8_project64(cam1, X) - np.array([float(kp1[0]), float(kp1[1])])
    mg["chi1"], mg["_e1"] = abs(math.hypot(*e1) - math.sqrt(5.991 * s1)), math.hypot(*e1)
    if e1 @ e1 > 5.991 * s1:
        return "chi1", mg, None
    e2 = kb8_project64(cam2, X2) - np.array([float(kp2[0]), float(kp2[1])])
    mg["chi2"], mg["_e2"] = abs(math.hypot(*e2) - math.sqrt(5.991 * s2)), math.hypot(*e2)
    if e2 @ e2 > 5.991 * s2:
        return "chi2", mg, None
    mg["floor"] = abs(X[2] - float(f32(0.0001))) / zscale
    if not X[2] > float(f32(0.0001)):
        return "depth_floor", mg, None
    return "ok", mg, X


def fisheye_undecided(label, mg, tol="default"):
    """True when a gate this pair went through is closer than the decided margin."""
    for k, v in mg.items():
        if k[0] == "_":                                             # (a value, not a margin)
            continue
        lim = FISHEYE_MARGIN["cos"] if k == "cos" else FISHEYE_MARGIN["px"] if k in ("chi1", "chi2") else FISHEYE_MARGIN["z_c"][tol]
        if v < lim:
            return True
    return False


def fisheye_frame(kpL, dL, mono_left, kpR, dR, mono_right, cam1, cam2, R12, t12, sigma2, rules=FREF, newton_steps=None, tol="default"):
    """Frame::ComputeStereoFishEyeMatches on two tables in lapping order.  -> dict nmatches, l2r, r2l, depth, p3d (float64, -1 /
    zeros where unset), labels and margins per left lapping-area row, undecided."""
    nl, nr = len(kpL), len(kpR)
    l2r, r2l = np.full(nl, -1, np.int64), np.full(nr, -1, np.int64)
    depth, p3d = np.full(nl, -1.0), np.zeros((nl, 3))
    labels, margins, undecided = [], [], 0
    nt = nr - mono_right
    for li in range(mono_left, nl):
        if nt < 2:                                                  # knnMatch returns fewer than two neighbours
            labels.append("ratio"); margins.append({}); continue
        d = hm.hamming(dL[li][None], dR[mono_right:])
        order = np.argsort(d, kind="stable")                        # first minimum first
        ri = int(order[0]) + mono_right
        lab, mg, X = fisheye_expect((kpL["x"][li], kpL["y"][li], kpL["octave"][li]), (kpR["x"][ri], kpR["y"][ri], kpR["octave"][ri]),
                                    cam1, cam2, R12, t12, sigma2, int(d[order[0]]), int(d[order[1]]), rules, newton_steps)
        labels.append(lab); margins.append(mg)
        undecided += fisheye_undecided(lab, mg, tol)
        if lab == "ok":
            l2r[li] = ri
            if not (rules.first_left_keeps_right and r2l[ri] >= 0):
                r2l[ri] = li
            depth[li], p3d[li] = X[2], X
    return {"nmatches": int((l2r >= 0).sum()), "l2r": l2r, "r2l": r2l, "depth": depth, "p3d": p3d, "labels": labels,
            "margins": margins, "undecided": undecided}


# ---- rigs ----
TUMVI_KB8 = ([190.978477, 190.973307, 254.931706, 256.897442, 0.00348238940, 0.000715034845, -0.00205323614, 0.000202936736],
             [190.442369, 190.434438, 252.597254, 254.917230, 0.00340031805, 0.00176627874, -0.00266312161, 0.000329951911])
PINHOLE_KB8 = [435.2, 435.2, 367.2, 252.2, 1 / 3, 2 / 15, 17 / 315, 62 / 2835]


def _roty(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])


RIGS = {
    # the two rigs of tests/test_gpu_parity.py
    "tumvi": (TUMVI_KB8[0], TUMVI_KB8[1], _roty(2.0).astype(f32), np.array([0.101, 0.002, -0.001], f32)),
    "pinhole": (PINHOLE_KB8, PINHOLE_KB8, _roty(0.05).astype(f32), np.array([0.11, 0.0004, -0.0003], f32)),
    # the TUM-VI rig shrunk 10^4 times: the geometry is the same, the depths straddle the 0.0001 floor of Frame.cc:1609
    "micro": (TUMVI_KB8[0], TUMVI_KB8[1], _roty(2.0).astype(f32), np.array([0.101e-4, 0.002e-4, -0.001e-4], f32)),
    # the second camera looks 90 degrees to the side: rays that meet in front of camera 1 and BEHIND camera 2 exist
    "wide": (TUMVI_KB8[0], TUMVI_KB8[1], _roty(90.0).astype(f32), np.array([0.101, 0.002, -0.001], f32)),
    # the second camera looks backwards and its r(theta) = theta (1 - theta^2 / pi^2) folds back to 0 at theta = pi: a point BEHIND it
    # on its axis projects within a few pixels of where the ray in front of it does, so the second chi-square gate lets it through
    # at octave 7 and only `z2 <= 0` refuses it -- the one place where that gate is not covered by the reprojection test after it
    "fold": (TUMVI_KB8[0], [190.0, 190.0, 252.0, 254.0, -1.0 / math.pi ** 2, 0.0, 0.0, 0.0], _roty(170.0).astype(f32),
             np.array([0.101, 0.002, -0.001], f32)),
}


def _pair_from_point(rig, X1):
    cam1, cam2, R12, t12 = RIGS[rig]
    _, T21 = rig_T21(R12, t12)
    return kb8_project64(cam1, X1), kb8_project64(cam2, T21[:3] @ np.append(X1, 1.0))


def _direction(rng, th_lo, th_hi):
    th, ph = rng.uniform(th_lo, th_hi), rng.uniform(0, 2 * np.pi)
    return np.array([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)])


def fisheye_cases(rig, seed, n_ok=0, n_far=0, n_rev=0, n_noise=0, n_corner=0, n_z2=0, n_centre=0, depth_scale=1.0, z2_on_axis=False):
    """Constructed pairs for one rig: dicts with kp1, kp2 = (x, y, octave), kind, P (the generating point, or None when the pair is
    not the image of one point), noise_free."""
    rng = np.random.default_rng(seed)
    cam1, cam2, R12, t12 = RIGS[rig]
    T12, T21 = rig_T21(R12, t12)
    sigma2 = fisheye_sigma2()
    out = []

    def octs():
        a = int(rng.integers(0, 8))
        return a, int((a + rng.integers(1, 8)) % 8)                 # different octaves in the two eyes

    def add(kind, p1, p2, P, noise_free):
        o1, o2 = octs()
        out.append({"kind": kind, "kp1": (f32(p1[0]), f32(p1[1]), o1), "kp2": (f32(p2[0]), f32(p2[1]), o2), "P": P,
                    "noise_free": noise_free})

    for _ in range(n_ok):                                           # 0.4 - 4 m: accepted
        X = _direction(rng, 0.02, 0.9) * rng.uniform(0.4, 4.0) * depth_scale
        add("ok", *_pair_from_point(rig, X), X, True)
    for _ in range(n_centre):                                       # left keypoint at the principal point: theta_d <= 1e-8
        X = np.array([0.0, 0.0, rng.uniform(0.5, 3.0) * depth_scale])
        p1, p2 = _pair_from_point(rig, X)
        add("centre", (f32(cam1[2]), f32(cam1[3])), p2, X, True)
    for _ in range(n_corner):                                       # towards the image corner: theta_d 1.2 .. 1.4
        X = _direction(rng, 1.2, 1.36) * rng.uniform(0.4, 1.5) * depth_scale
        add("corner", *_pair_from_point(rig, X), X, True)
    for _ in range(n_far):                                          # 3 - 12 m: straddles cos = 0.9998 for a 0.1 m baseline
        X = _direction(rng, 0.02, 0.7) * rng.uniform(3.0, 12.0) * depth_scale
        add("far", *_pair_from_point(rig, X), X, True)
    for _ in range(n_rev):                                          # the right keypoint 20 - 60 px beyond its point at infinity
        d = _direction(rng, 0.05, 0.8)
        X = d * rng.uniform(0.5, 3.0) * depth_scale
        p1, p2 = _pair_from_point(rig, X)
        pinf = kb8_project64(cam2, T21[:3, :3] @ d)
        e = (pinf - p2) / np.linalg.norm(pinf - p2)
        add("reversed", p1, pinf + e * rng.uniform(20, 60), None, False)
    for _ in range(n_noise):                                        # pixel noise around the chi-square limit, one eye at a time
        X = _direction(rng, 0.02, 0.8) * rng.uniform(0.4, 2.5) * depth_scale
        p1, p2 = _pair_from_point(rig, X)
        o1, o2 = octs()
        eye = int(rng.integers(2))
        ph = rng.uniform(0, 2 * np.pi)
        amp = rng.uniform(0.8, 3.4) * math.sqrt(5.991 * float(sigma2[min(o1, o2)]))
        dv = amp * np.array([np.cos(ph), np.sin(ph)])
        if eye == 0:
            p1 = p1 + dv
        else:
            p2 = p2 + dv
        out.append({"kind": "noise", "kp1": (f32(p1[0]), f32(p1[1]), o1), "kp2": (f32(p2[0]), f32(p2[1]), o2), "P": None,
                    "noise_free": False})
    for _ in range(n_z2):                                           # rays that meet behind camera 2 and in front of camera 1
        while True:
            if z2_on_axis:                                          # 1 - 2.5 px from camera 2's principal point
                rr, ph = rng.uniform(1.0, 2.5), rng.uniform(0, 2 * np.pi)
                r2 = kb8_unproject64(cam2, f32(cam2[2]) + rr * np.cos(ph), f32(cam2[3]) + rr * np.sin(ph))
            else:
                r2 = kb8_unproject64(cam2, rng.uniform(60, 450), rng.uniform(60, 450))
            X2 = -rng.uniform(0.3, 2.0) * r2
            X = T12[:3] @ np.append(X2, 1.0)
            if X[2] > 0.2 and math.atan2(math.hypot(X[0], X[1]), X[2]) < 1.2:
                break
        p2 = kb8_project64(cam2, r2)
        add("behind_cam2", kb8_project64(cam1, X), p2, None, False)
        if z2_on_axis:
            out[-1]["kp2"] = out[-1]["kp2"][:2] + (7,)
            out[-1]["kp1"] = out[-1]["kp1"][:2] + (int(rng.integers(0, 7)),)
    return out


def fisheye_sigma2(nlevels=8, scale=1.2):
    sf, _ = hm.scale_factors(nlevels, scale)
    return (sf * sf).astype(f32)                                    # mvLevelSigma2, ORBextractor.cc:424


def fisheye_table(name, rig, cases, seed, mono_left=6, mono_right=9, ratio=(), dup=None, shuffle=True, tol="default"):
    """Two tables in lapping order from constructed pairs.  Left lapping row i carries code row i; its partner on the right is
    that row with d0 bits flipped (ratio[i] = (d0, d1): d0 flips, and a second right row with d1 flips somewhere else in the
    image); the mono rows in front of both tables repeat left descriptors EXACTLY, so a lost mono offset is seen.  dup = (i, k):
    k rows after the end of the left table, row i once more (same keypoint, same descriptor)."""
    rng = np.random.default_rng(seed)
    n = len(cases)
    codes = code_rows(n, 0) if n else np.zeros((0, 32), np.uint8)
    ratio = dict(ratio)
    kpl = np.zeros(n, KEYPOINT_DT); kpr_rows, dr_rows = [], []
    for i, c in enumerate(cases):
        kpl["x"][i], kpl["y"][i], kpl["octave"][i] = c["kp1"]
        d0, d1 = ratio.get(i, (int(rng.integers(0, 6)), None))
        kpr_rows.append(c["kp2"]); dr_rows.append(flip_bits(codes[i], d0, rng))
        if d1 is not None:
            kpr_rows.append((f32(rng.uniform(100, 400)), f32(rng.uniform(100, 400)), int(rng.integers(0, 8))))
            dr_rows.append(flip_bits(codes[i], d1, rng))
    dl = codes
    if dup is not None:
        i, k = dup
        fill = np.zeros(k, KEYPOINT_DT)
        fill["x"], fill["y"] = rng.uniform(100, 400, k), rng.uniform(100, 400, k)
        kpl = np.concatenate([kpl, fill, kpl[i:i + 1]])
        dl = np.concatenate([dl, code_rows(k, 512 - k), dl[i:i + 1]])   # (fillers: rows no right descriptor is near)
    nrr = len(kpr_rows)
    kpr = np.zeros(nrr, KEYPOINT_DT)
    for j, r in enumerate(kpr_rows):
        kpr["x"][j], kpr["y"][j], kpr["octave"][j] = r
    dr = np.array(dr_rows, np.uint8).reshape(nrr, 32)
    if shuffle and nrr:
        perm = rng.permutation(nrr)
        kpr, dr = kpr[perm], dr[perm]
    def mono(k, src_d):
        m = np.zeros(k, KEYPOINT_DT)
        m["x"], m["y"], m["octave"] = rng.uniform(0, 40, k), rng.uniform(0, 400, k), rng.integers(0, 8, k)
        d = src_d[rng.integers(0, len(src_d), k)] if len(src_d) else code_rows(k, 300)
        return m, d
    ml, mdl = mono(mono_left, dr if nrr else dl)                     # left mono rows repeat RIGHT descriptors and vice versa
    mr, mdr = mono(mono_right, dl if len(dl) else dr)
    cam1, cam2, R12, t12 = RIGS[rig]
    T = {"name": name, "rig": rig, "cases": cases, "kpL": np.concatenate([ml, kpl]), "dL": np.concatenate([mdl, dl]).astype(np.uint8),
         "monoL": mono_left, "kpR": np.concatenate([mr, kpr]), "dR": np.concatenate([mdr, dr]).astype(np.uint8), "monoR": mono_right,
         "cam1": cam1, "cam2": cam2, "R": R12, "t": t12, "tol": tol}
    T["expect"] = run_fisheye(T)
    T["refused"] = T["expect"]["undecided"]
    return T


def run_fisheye(T, rules=FREF, newton_steps=None):
    return fisheye_frame(T["kpL"], T["dL"], T["monoL"], T["kpR"], T["dR"], T["monoR"], T["cam1"], T["cam2"], T["R"], T["t"],
                         fisheye_sigma2(), rules, newton_steps, T["tol"])


_FISHEYE = None


def fisheye_corpus():
    """The committed fisheye tables (built once per process)."""
    global _FISHEYE
    if _FISHEYE is not None:
        return _FISHEYE
    out = []
    main = fisheye_cases("tumvi", 31, n_ok=60, n_far=70, n_rev=14, n_noise=150, n_centre=3)
    ratio = {0: (7, 10), 1: (6, 10), 2: (70, 100), 3: (69, 100), 4: (0, 0), 5: (14, 20), 6: (13, 20), 7: (35, 50), 8: (3, 5)}
    out.append(fisheye_table("tumvi_main", "tumvi", main, 41, ratio=ratio, dup=(12, 70)))
    out.append(fisheye_table("pinhole", "pinhole", fisheye_cases("pinhole", 32, n_ok=40, n_far=40, n_rev=6, n_noise=40), 42))
    out.append(fisheye_table("micro", "micro", fisheye_cases("micro", 67, n_ok=50, depth_scale=1e-4), 43))
    out.append(fisheye_table("wide", "wide", fisheye_cases("wide", 34, n_z2=12), 44))
    out.append(fisheye_table("fold", "fold", fisheye_cases("fold", 36, n_z2=8, z2_on_axis=True), 45))
    # keypoints towards the image corner: the depth is a fraction of the range, so the z-based unit of the tolerance is small for
    # them and their measured c is recorded on its own
    out.append(fisheye_table("tumvi_corner", "tumvi", fisheye_cases("tumvi", 37, n_corner=16, n_ok=4), 46, tol="corner"))
    # shapes: 63 / 64 / 65 left lapping rows, 0 / 1 / 2 right lapping rows, an empty left lapping area
    ok = fisheye_cases("tumvi", 35, n_ok=40, n_far=15, n_noise=10)
    for n in (63, 64, 65):
        out.append(fisheye_table("lap%d" % n, "tumvi", ok[:n], 50 + n, mono_left=n % 5, mono_right=3))
    two = fisheye_table("nr2", "tumvi", ok[:2], 60)
    out.append(two)
    for nr in (0, 1):
        T = dict(two)
        T["name"] = "nr%d" % nr
        T["kpR"], T["dR"] = two["kpR"][:two["monoR"] + nr], two["dR"][:two["monoR"] + nr]
        T["expect"] = run_fisheye(T)
        out.append(T)
    T = dict(out[4])
    T["name"], T["monoL"] = "mono_left_is_nleft", len(T["kpL"])
    T["expect"] = run_fisheye(T)
    out.append(T)
    _FISHEYE = out
    return out
