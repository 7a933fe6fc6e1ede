"""The front of Tracking::SearchLocalPointsAndLines (Tracking.cc:3809-3883) for a frame of one camera, restated in numpy, CPU only:
Frame::isInFrustum (Frame.cc:585-647) and Frame::isInFrustum_l (:661-701) in np.float32 in the reference's operation order (a
cv::Mat product: double accumulation, one rounding; cv::norm and Mat::dot summed in double), the queries of ORBmatcher.cc:53-73,
then helpers_matchers.search_local_map / match_nnr, which tests/test_ref_pin_match.py pins to the reference's own code.
tests/test_local_map_gpu.py compares pli_search_local_points / pli_search_local_lines with these byte for byte.

`misread` names deliberate misreadings that tests/test_local_map_cpu.py wants its constructed rows to reject:
  "image_half_open"  the image gate of KeyFrame::IsInImage (open at mnMaxX / mnMaxY) instead of Frame.cc:607-610
  "nan_out"          a gate written as !(u >= min && u <= max): a NaN projection leaves
  "normal_double"    the viewing angle as Fuse tests it, dot < 0.5 * dist in double (ORBmatcher.cc:1492)
  "pinhole_form"     the line's projection as Pinhole::project rounds it, fx*x/z + cx
  "invz_form"        the point's projection as isInFrustum_l rounds it, fx*x*invz + cx"""
import math
from collections import Counter

import numpy as np

import helpers_matchers as hm
from test_fuse_search_cpu import CAM, FUSE_POINT_DT, NLEVELS, SF, gemm_row, level_ratio

f32, f64 = np.float32, np.float64
LOCAL_VIEW_DT = np.dtype([("proj_x", "<f4"), ("proj_y", "<f4"), ("proj_xr", "<f4"), ("depth", "<f4"), ("view_cos", "<f4"),
                          ("level", "<i4"), ("in_view", "<i4"), ("pad", "<i4")])
POINT_EXITS = ("not_valid", "neg_depth", "left", "right", "top", "bottom", "too_near", "too_far", "view_angle", "in_view")
LINE_EXITS = ("not_valid", "neg_depth", "left", "right", "top", "bottom", "in_view")
STORED_VIEW = 2                                            # PLI_LOCAL_STORED_VIEW
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0], f32)


def _norm3(a):
    """cv::norm of a 3-vector of floats: the squares summed in double, the root rounded to float."""
    return f32(math.sqrt(float(a[0]) * float(a[0]) + float(a[1]) * float(a[1]) + float(a[2]) * float(a[2])))


def _outside(u, lo, hi, misread):
    """-> None inside, else "lo" / "hi"; Frame.cc:607-610 as written (a NaN compares false twice and stays)."""
    if "nan_out" in misread and not (u >= lo and u <= hi):
        return "lo" if u < lo else "hi"
    if u < lo:
        return "lo"
    if u > hi or ("image_half_open" in misread and u == hi):
        return "hi"
    return None


def is_in_frustum(points, pose, cam=CAM, limit=0.5, lr=None, exits=None, misread=()):
    """Frame::isInFrustum of every row of points (FUSE_POINT_DT) -> LOCAL_VIEW_DT rows as pli_search_local_points defines them."""
    lr = level_ratio() if lr is None else lr
    exits = exits if exits is not None else Counter()
    R, t, Ow = pose[:9].reshape(3, 3), pose[9:12], pose[12:15]
    view = np.zeros(len(points), LOCAL_VIEW_DT)
    limit = f32(limit)
    with np.errstate(all="ignore"):
        for i, P in enumerate(points):
            V = view[i]
            if P["valid"] == STORED_VIEW:                            # skipped at Tracking.cc:3813, searched by ORBmatcher.cc:53
                exits["stored_view"] += 1; continue
            if not P["valid"]:
                exits["not_valid"] += 1; continue
            V["proj_x"] = V["proj_y"] = -1.0
            p = P["pos"]
            x, y, z = (gemm_row(R[r], p, t[r]) for r in range(3))
            pc_dist = _norm3((x, y, z))
            invz = f32(f32(1.0) / z)
            if z < f32(0.0):
                exits["neg_depth"] += 1; continue
            if "invz_form" in misread:
                u = f32(f32(f32(cam.fx * x) * invz) + cam.cx)
                v = f32(f32(f32(cam.fy * y) * invz) + cam.cy)
            else:
                u = f32(f32(f32(cam.fx * x) / z) + cam.cx)
                v = f32(f32(f32(cam.fy * y) / z) + cam.cy)
            side = _outside(u, cam.min_x, cam.max_x, misread)
            if side:
                exits["left" if side == "lo" else "right"] += 1; continue
            side = _outside(v, cam.min_y, cam.max_y, misread)
            if side:
                exits["top" if side == "lo" else "bottom"] += 1; continue
            V["proj_x"], V["proj_y"] = u, v
            PO = (p - Ow).astype(f32)
            dist = _norm3(PO)
            if dist < P["min_dist_inv"]:
                exits["too_near"] += 1; continue
            if dist > P["max_dist_inv"]:
                exits["too_far"] += 1; continue
            Pn = P["normal"]
            dot = float(PO[0]) * float(Pn[0]) + float(PO[1]) * float(Pn[1]) + float(PO[2]) * float(Pn[2])
            view_cos = f32(f64(dot) / f64(dist))
            if (dot < 0.5 * float(dist)) if "normal_double" in misread else (view_cos < limit):
                exits["view_angle"] += 1; continue
            ratio = f32(P["max_dist"] / dist)
            V["level"] = int((ratio > lr).sum())
            V["in_view"] = 1
            V["proj_xr"] = f32(u - f32(cam.bf * invz))
            V["depth"] = pc_dist
            V["view_cos"] = view_cos
            exits["in_view"] += 1
    return view


def stored_view(proj_x, proj_y, proj_xr, depth, view_cos, level):
    """The pli_fuse_point row of a point that Tracking.cc:3813 skips and that still has mbTrackInView set (PLI_LOCAL_STORED_VIEW):
    it carries the fields the point holds, and ORBmatcher.cc:53-73 searches it with them."""
    P = np.zeros(1, FUSE_POINT_DT)
    P["pos"], P["normal"], P["valid"] = (proj_x, proj_y, proj_xr), (depth, view_cos, level), STORED_VIEW
    return P


def local_queries(view, th=1.0, far_points=False, th_far=0.0, sf=SF, points=None):
    """The queries of ORBmatcher::SearchByProjection(F, vpMapPoints, th, bFarPoints, thFarPoints), ORBmatcher.cc:53-73, from the
    records of the points in view and from the stored fields of the rows of `points` marked STORED_VIEW.  A query whose projection
    is NaN takes no keypoint (every |x - u| < r of GetFeaturesInArea is false; the cell range the reference derives from it is a
    float-to-int conversion of NaN): it is closed here, as the device closes it."""
    q = np.zeros(len(view), hm.PROJ_QUERY_DT)
    th = f32(th)
    for i, V in enumerate(view):
        if points is not None and points[i]["valid"] == STORED_VIEW:
            P = points[i]
            x, y, xr, depth, cos, lv = P["pos"][0], P["pos"][1], P["pos"][2], P["normal"][0], P["normal"][1], int(P["normal"][2])
        elif V["in_view"]:
            x, y, xr, depth, cos, lv = V["proj_x"], V["proj_y"], V["proj_xr"], V["depth"], V["view_cos"], int(V["level"])
        else:
            continue
        if far_points and depth > f32(th_far):
            continue
        r = f32(2.5) if float(cos) > 0.998 else f32(4.0)                     # RadiusByViewingCos: the float against a double
        if th != f32(1.0):
            r = f32(r * th)
        q[i] = (x, y, f32(r * sf[lv]), xr, lv - 1, lv, 0.0, 0 if (np.isnan(x) or np.isnan(y)) else 1)
    return q


def search_local_points(points, descs, pose, kp, desc, uright, occupied, cam=CAM, th=1.0, far_points=False, th_far=0.0,
                        nnratio=0.8, limit=0.5, exits=None, misread=(), lr=None):
    """-> view, best_idx2, n_in_view, nmatches, queries.  lr: the level_ratio table (default: test_fuse_search_cpu.level_ratio)."""
    view = is_in_frustum(points, pose, cam, limit, lr=lr, exits=exits, misread=misread)
    q = local_queries(view, th, far_points, th_far, points=points)
    bounds = (cam.min_x, cam.max_x, cam.min_y, cam.max_y)
    n, best, _ = hm.search_local_map(q, descs, kp, desc, uright, occupied, bounds, nnratio)
    return view, best, int(view["in_view"].sum()), n, q


def is_in_frustum_l(sp, valid, pose, cam=CAM, exits=None, misread=()):
    """Frame::isInFrustum_l of every start point -> in_view[nl] (int32), proj_s[nl, 2] (0 where not in view)."""
    exits = exits if exits is not None else Counter()
    R, t = pose[:9].reshape(3, 3), pose[9:12]
    nl = len(sp)
    in_view, proj = np.zeros(nl, np.int32), np.zeros((nl, 2), f32)
    with np.errstate(all="ignore"):
        for i in range(nl):
            if not valid[i]:
                exits["not_valid"] += 1; continue
            x, y, z = (gemm_row(R[r], sp[i], t[r]) for r in range(3))
            if z < f32(0.0):
                exits["neg_depth"] += 1; continue
            invz = f32(f32(1.0) / z)
            if "pinhole_form" in misread:
                u = f32(f32(f32(cam.fx * x) / z) + cam.cx)
                v = f32(f32(f32(cam.fy * y) / z) + cam.cy)
            else:
                u = f32(f32(f32(cam.fx * x) * invz) + cam.cx)
                v = f32(f32(f32(cam.fy * y) * invz) + cam.cy)
            side = _outside(u, cam.min_x, cam.max_x, misread)
            if side:
                exits["left" if side == "lo" else "right"] += 1; continue
            side = _outside(v, cam.min_y, cam.max_y, misread)
            if side:
                exits["top" if side == "lo" else "bottom"] += 1; continue
            in_view[i] = 1
            proj[i] = (u, v)
            exits["in_view"] += 1
    return in_view, proj


def search_local_lines(sp, valid, descs, pose, cur_desc, nnr, cam=CAM, exits=None, misread=()):
    """-> in_view, proj_s, in_frustum, matches_12, nmatches."""
    in_view, proj = is_in_frustum_l(sp, valid, pose, cam, exits, misread)
    lst = np.flatnonzero(in_view).astype(np.int32)
    n, m = hm.match_nnr(descs[lst], cur_desc, nnr) if len(lst) else (0, np.zeros(0, np.int32))
    return in_view, proj, lst, m, n


def host_line_gate(lst, matches_12, proj_s, proj_e, kl_start, kl_end, disparity, occupied, nobs, bounds):
    """The loop Tracking.cc:3886-3919 on the fields as they stand (proj_e: mTrackProjeX / Y of every map line, which the reference
    never writes) -> matches_12 after the position gate, and {frame line: list index} as mvpMapLines is left.  occupied: the frame
    lines that hold a map line with observations at entry; a line written by the loop holds its row against the matches behind it
    when it has observations itself (nobs, per map line), and is overwritten otherwise."""
    dw = (float(bounds[1]) - float(bounds[0])) * 0.1
    dh = (float(bounds[3]) - float(bounds[2])) * 0.1
    out, assigned = matches_12.copy(), {}
    occupied = np.array(occupied, bool)
    for i1, i2 in enumerate(matches_12):
        if i2 < 0:
            continue
        if disparity[i2][0] < 0 or disparity[i2][1] < 0:
            continue
        if occupied[i2]:
            continue
        li = lst[i1]
        if (abs(float(f32(kl_start[i2][0] - proj_s[li][0]))) > dw or abs(float(f32(kl_end[i2][0] - proj_e[li][0]))) > dw or
                abs(float(f32(kl_start[i2][1] - proj_s[li][1]))) > dh or abs(float(f32(kl_end[i2][1] - proj_e[li][1]))) > dh):
            out[i1] = -1
            continue
        assigned[int(i2)] = int(li)
        occupied[i2] = nobs[li] > 0
    return out, assigned


def canonical(a):
    """The bytes of a record array with every NaN replaced by one NaN: which NaN an invalid operation returns (sign, payload) is
    not fixed by IEEE 754 and differs between processors, the reference's own host included."""
    a = np.array(a, copy=True)
    names = a.dtype.names or (None,)
    for nme in names:
        col = a[nme] if nme else a
        if col.dtype.kind == "f":
            col[np.isnan(col)] = np.nan
    return a.tobytes()


# ---- scenes ---------------------------------------------------------------------------------------------------------------------

def rot(a, b, c):
    ca, sa, cb, sb, cc, sc = math.cos(a), math.sin(a), math.cos(b), math.sin(b), math.cos(c), math.sin(c)
    Rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]])
    Ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    Rz = np.array([[cc, -sc, 0], [sc, cc, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def make_pose(rng):
    R = rot(*rng.uniform(-0.2, 0.2, 3))
    t = rng.uniform(-1.0, 1.0, 3)
    return np.concatenate([R.reshape(-1), t, -R.T @ t]).astype(f32)


def _world(pose, u, v, z, cam):
    """float64: the world point whose camera coordinates are ((u - cx) z / fx, (v - cy) z / fy, z)."""
    R, t = pose[:9].reshape(3, 3).astype(f64), pose[9:12].astype(f64)
    pc = np.stack([(u - float(cam.cx)) * z / float(cam.fx), (v - float(cam.cy)) * z / float(cam.fy), z], -1)
    return (pc - t) @ R                                              # R^T (pc - t), row-wise


def make_points(rng, pose, nq, cam=CAM):
    """Map points that take every exit of isInFrustum: pixels drawn from a frame 60 px wider than the image on every side, one in
    sixteen behind the camera, the distance range off for one in eight, the normal up to 75 degrees from the ray (two in five
    within 3 degrees: view_cos on both sides of 0.998), every level predicted."""
    u = rng.uniform(float(cam.min_x) - 60, float(cam.max_x) + 60, nq)
    v = rng.uniform(float(cam.min_y) - 60, float(cam.max_y) + 60, nq)
    z = rng.uniform(0.5, 20.0, nq) * np.where(rng.random(nq) < 1 / 16, -1.0, 1.0)
    pw = _world(pose, u, v, z, cam)
    po = pw - pose[12:15].astype(f64)
    dist = np.linalg.norm(po, axis=1)
    ray = po / dist[:, None]
    ang = np.where(rng.random(nq) < 0.4, rng.uniform(0, math.radians(3), nq), rng.uniform(math.radians(3), math.radians(75), nq))
    side = np.cross(ray, rng.normal(size=(nq, 3)))
    side /= np.linalg.norm(side, axis=1)[:, None]
    normal = ray * np.cos(ang)[:, None] + side * np.sin(ang)[:, None]
    level = rng.integers(0, NLEVELS, nq)
    max_dist = dist * 1.2 ** (level - 0.5)
    pts = np.zeros(nq, FUSE_POINT_DT)
    pts["pos"], pts["normal"] = pw, normal
    pts["max_dist"] = max_dist
    pts["max_dist_inv"] = 1.2 * max_dist
    pts["min_dist_inv"] = 0.2 * max_dist
    k = rng.random(nq)
    pts["max_dist_inv"] = np.where(k < 1 / 16, 0.9 * dist, pts["max_dist_inv"])       # too far
    pts["min_dist_inv"] = np.where(k > 15 / 16, 1.1 * dist, pts["min_dist_inv"])      # too near
    pts["valid"] = rng.random(nq) < 0.93
    descs = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    return pts, descs


def make_frame(rng, view, descs, ncur, cam=CAM):
    """A frame around the points in view: most keypoints lie within a few pixels of a projection, on the predicted level or next
    to it, with the point's descriptor and a few bits flipped; half carry a right coordinate, one in ten holds a map point."""
    kp = np.zeros(ncur, hm.KEYPOINT_DT)
    desc = rng.integers(0, 256, (ncur, 32), dtype=np.uint8)
    kp["x"] = rng.uniform(float(cam.min_x), float(cam.max_x), ncur)
    kp["y"] = rng.uniform(float(cam.min_y), float(cam.max_y), ncur)
    kp["octave"] = rng.integers(0, NLEVELS, ncur)
    kp["angle"] = rng.uniform(0, 360, ncur)
    ur = np.full(ncur, -1.0, f32)
    seen = np.flatnonzero(view["in_view"] & np.isfinite(view["proj_x"]) & np.isfinite(view["proj_y"]))
    if len(seen) and ncur:
        near = rng.random(ncur) < 0.8
        src = seen[rng.integers(0, len(seen), ncur)]
        kp["x"] = np.where(near, view["proj_x"][src] + rng.uniform(-5, 5, ncur), kp["x"])
        kp["y"] = np.where(near, view["proj_y"][src] + rng.uniform(-5, 5, ncur), kp["y"])
        kp["octave"] = np.where(near, np.clip(view["level"][src] - rng.integers(-1, 3, ncur), 0, NLEVELS - 1), kp["octave"])
        d = descs[src].copy()
        flip = rng.random((ncur, 32)) < 0.08
        d[flip] ^= rng.integers(1, 256, (ncur, 32), dtype=np.uint8)[flip]
        desc = np.where(near[:, None], d, desc)
        stereo = near & (rng.random(ncur) < 0.5)
        ur = np.where(stereo, view["proj_xr"][src] + rng.uniform(-6, 6, ncur), ur).astype(f32)
    occ = (rng.random(ncur) < 0.1).astype(np.uint8)
    return kp, np.ascontiguousarray(desc), ur, occ


_SCENES = {}


def point_scene(seed, nq, ncur):
    """-> pose, points, descs, kp, desc, uright, occupied; made once per (seed, nq, ncur) and shared: do not write to it."""
    key = ("p", seed, nq, ncur)
    if key not in _SCENES:
        rng = np.random.default_rng(seed)
        pose = make_pose(rng)
        pts, descs = make_points(rng, pose, nq)
        view = is_in_frustum(pts, pose)
        _SCENES[key] = (pose, pts, descs) + make_frame(rng, view, descs, ncur)
    return _SCENES[key]


def line_scene(seed, nl, n2, cam=CAM):
    """-> pose, sp, valid, descs, cur_desc; the frame's lines carry the descriptors of map lines with a few bits flipped."""
    key = ("l", seed, nl, n2)
    if key not in _SCENES:
        rng = np.random.default_rng(seed)
        pose = make_pose(rng)
        u = rng.uniform(float(cam.min_x) - 80, float(cam.max_x) + 80, nl)
        v = rng.uniform(float(cam.min_y) - 80, float(cam.max_y) + 80, nl)
        z = rng.uniform(0.5, 20.0, nl) * np.where(rng.random(nl) < 1 / 12, -1.0, 1.0)
        sp = _world(pose, u, v, z, cam).astype(f32).reshape(nl, 3)
        valid = (rng.random(nl) < 0.9).astype(np.uint8)
        descs = rng.integers(0, 256, (nl, 32), dtype=np.uint8)
        cur = rng.integers(0, 256, (n2, 32), dtype=np.uint8)
        if nl and n2:
            src = rng.integers(0, nl, n2)
            cur = descs[src].copy()
            flip = rng.random((n2, 32)) < 0.1
            cur[flip] ^= rng.integers(1, 256, (n2, 32), dtype=np.uint8)[flip]
        _SCENES[key] = (pose, sp, valid, descs, np.ascontiguousarray(cur))
    return _SCENES[key]


# ---- constructed rows (identity pose: the camera point IS the world point, Rcw * p + tcw is exact) ---------------------------

def one_point(pos, normal=(0.0, 0.0, 1.0), max_dist=None):
    P = np.zeros(1, FUSE_POINT_DT)
    P["pos"], P["normal"] = pos, normal
    d = float(np.linalg.norm(np.asarray(pos, f64)))
    P["max_dist"] = max_dist if max_dist is not None else max(d, 1.0)
    P["min_dist_inv"], P["max_dist_inv"] = 0.0, 1e9
    P["valid"] = 1
    return P


def _ulps(x, k):
    return (np.array([x], f32).view(np.int32) + k).view(f32)[0]


def point_on_the_far_corner(cam=CAM, seed=5):
    """A point whose projection is (mnMaxX, mnMaxY) exactly, found by stepping x and y through neighbouring floats."""
    rng = np.random.default_rng(seed)
    for _ in range(200):
        z = f32(rng.uniform(1.0, 8.0))
        out = []
        for f, c, hi in ((cam.fx, cam.cx, cam.max_x), (cam.fy, cam.cy, cam.max_y)):
            x0 = f32((float(hi) - float(c)) * float(z) / float(f))
            hit = [x for x in (_ulps(x0, k) for k in range(-64, 65)) if f32(f32(f32(f * x) / z) + c) == hi]
            if hit:
                out.append(hit[0])
        if len(out) == 2:
            return one_point((out[0], out[1], z), normal=np.array([out[0], out[1], z], f64) / np.linalg.norm([out[0], out[1], z]))
    raise AssertionError("no point projects onto (mnMaxX, mnMaxY)")


def point_where_the_angle_tests_disagree(cam=CAM, seed=9):
    """In view by Frame.cc:627-629 (viewCos rounds to 0.5f, not < 0.5f), refused by dot < 0.5 * dist in double."""
    rng = np.random.default_rng(seed)
    for _ in range(200000):
        pos = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(2, 6)]).astype(f32)
        ray = pos.astype(f64) / np.linalg.norm(pos.astype(f64))
        side = np.cross(ray, rng.normal(size=3)); side /= np.linalg.norm(side)
        n = (ray * 0.5 + side * math.sqrt(0.75)).astype(f32)
        dist = _norm3(pos)
        dot = float(pos[0]) * float(n[0]) + float(pos[1]) * float(n[1]) + float(pos[2]) * float(n[2])
        if f32(f64(dot) / f64(dist)) == f32(0.5) and dot < 0.5 * float(dist):
            return one_point(pos, normal=n)
    raise AssertionError("no point found")


def line_where_the_two_forms_disagree(cam=CAM, seed=3):
    """A start point with fx*X*invz + cx <= mnMaxX (in view) and fx*X/z + cx > mnMaxX, or the other way round."""
    rng = np.random.default_rng(seed)
    for _ in range(20000):
        z = f32(rng.uniform(1.0, 8.0))
        invz = f32(f32(1.0) / z)
        x0 = f32((float(cam.max_x) - float(cam.cx)) * float(z) / float(cam.fx))
        for k in range(-64, 65):
            x = _ulps(x0, k)
            a = f32(f32(f32(cam.fx * x) * invz) + cam.cx)
            b = f32(f32(f32(cam.fx * x) / z) + cam.cx)
            if (a > cam.max_x) != (b > cam.max_x):
                return np.array([[x, 0.0, z]], f32)
    raise AssertionError("no line found")
