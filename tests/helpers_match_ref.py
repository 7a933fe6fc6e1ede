"""The matcher pin's corpus and fixtures: the searches of the reference's own src/ORBmatcher.cc, compiled where it lies into
oracle/_ref/pli_ref_match (oracle/Makefile: ref_match; the stand-in it compiles against is oracle/ref_recipe/match_shim), run over
the scenes and hand-built tables the CPU tests of every search already have.

  CASES                 the named cases, each one scene of one function: its input arrays, the calls it makes (one reference call
                        per keyframe / neighbour / candidate / setting) and what the restatement, the oracle and the device make
                        of the same arrays
  run_reference         one call of pli_ref_match as a child process
  save_fixture / load_fixture    tests/golden/match_ref/<case>.npz: "in/<array>" and "out/<call>/<array>"

tools/gen_match_ref.py writes the fixtures; tests/test_ref_pin_match.py and tests/test_ref_pin_match_gpu.py read them.  Nothing here
reads the reference tree; run_reference needs the program oracle/Makefile built from it.

Pointers travel as indices.  Every case allocates its MapPoints from one array, so that pointer order is index order.  By
convention here the MapPoint of list entry i is object i; the objects after the list are the ones tables hold at entry."""
import io
import os
import struct
import subprocess
import tempfile
import zipfile
from collections import Counter

import numpy as np

import helpers_matchers as HM
import test_bow_kf_search_cpu as BK
import test_bow_search_cpu as BW
import test_fuse_search_cpu as FU
import test_init_search_cpu as IN
import test_reloc_projection_cpu as RL
import test_sim3_projection_cpu as S3
import test_triangulation_search_cpu as TR
from helpers_matchers import KEYPOINT_DT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD_DIR = os.path.join(ROOT, "tests", "golden", "match_ref")
REF_EXE = os.path.join(ROOT, "oracle", "_ref", "pli_ref_match")
f32, f64 = np.float32, np.float64
LOGSF = f32(np.log(float(f32(FU.SCALE))))                              # mfLogScaleFactor as predict_scale takes it
SIGMA2 = (FU.SF * FU.SF).astype(f32)
OPS = {1: "GetDescriptor", 2: "GetMapPoint", 3: "Replace", 4: "AddObservation", 5: "AddMapPoint"}      # the driver's record of Fuse's calls
_TYPES = {np.dtype(np.uint8): 0, np.dtype(np.int32): 1, np.dtype(np.float32): 2, np.dtype(np.float64): 3}
_DTYPES = {v: k for k, v in _TYPES.items()}


# ------------------------------------------------------------------------------------------------- the driver's file format
def write_bag(path, bag):
    with open(path, "wb") as f:
        f.write(b"PLIM" + struct.pack("<i", len(bag)))
        for name in sorted(bag):
            a = np.ascontiguousarray(bag[name])
            f.write(struct.pack("<i", len(name)) + name.encode())
            f.write(struct.pack("<ii", _TYPES[a.dtype], a.ndim) + struct.pack("<%dq" % a.ndim, *a.shape))
            f.write(a.tobytes())


def read_bag(path):
    raw = open(path, "rb").read()
    assert raw[:4] == b"PLIM"
    (count,), o, bag = struct.unpack_from("<i", raw, 4), 8, {}
    for _ in range(count):
        (ln,) = struct.unpack_from("<i", raw, o); o += 4
        name = raw[o:o + ln].decode(); o += ln
        t, nd = struct.unpack_from("<ii", raw, o); o += 8
        shape = struct.unpack_from("<%dq" % nd, raw, o); o += 8 * nd
        a = np.frombuffer(raw, _DTYPES[t], int(np.prod(shape, dtype=np.int64)), o).reshape(shape).copy()
        o += a.nbytes
        bag[name] = a
    assert o == len(raw)
    return bag


def run_reference(bag, exe=REF_EXE):
    """One call of the reference program: the result arrays by name."""
    with tempfile.TemporaryDirectory() as d:
        req, rsp = os.path.join(d, "case"), os.path.join(d, "result")
        write_bag(req, bag)
        subprocess.run([exe, req, rsp], check=True, timeout=120)
        return read_bag(rsp)


# ---------------------------------------------------------------------------------------------------------------- fixtures
def fixture_path(name):
    return os.path.join(GOLD_DIR, name + ".npz")


def save_fixture(name, arrays, results):
    """A .npz whose bytes depend on its arrays alone (fixed entry dates, sorted names)."""
    os.makedirs(GOLD_DIR, exist_ok=True)
    flat = {"in/" + k: v for k, v in arrays.items()}
    for call, res in results.items():
        flat.update({"out/%s/%s" % (call, k): v for k, v in res.items()})
    with zipfile.ZipFile(fixture_path(name), "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(flat):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(flat[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


_FIX = {}


def load_fixture(name):
    """-> (arrays, {call: {array}}); read once, left unchanged."""
    if name not in _FIX:
        z = np.load(fixture_path(name))
        arrays, results = {}, {}
        for key in z.files:
            parts = key.split("/")
            if parts[0] == "in":
                arrays["/".join(parts[1:])] = z[key]
            else:
                results.setdefault(parts[1], {})[parts[2]] = z[key]
        for a in list(arrays.values()) + [v for r in results.values() for v in r.values()]:
            a.setflags(write=False)
        _FIX[name] = (arrays, results)
    return _FIX[name]


# ----------------------------------------------------------------------------------------------- tables of the driver's case
def cam10(cam, mb=0.0):
    return np.array([cam.fx, cam.fy, cam.cx, cam.cy, cam.bf, cam.min_x, cam.max_x, cam.min_y, cam.max_y, mb], f32)


def cam_of(c10):
    return FU.Cam(*[f32(v) for v in c10[:9]])


def table_bag(pre, x, y, octave, angle, desc, cam, **more):
    n = len(x)
    bag = {pre + "x": np.asarray(x, f32), pre + "y": np.asarray(y, f32), pre + "octave": np.asarray(octave, np.int32),
           pre + "angle": np.zeros(n, f32) if angle is None else np.asarray(angle, f32),
           pre + "desc": np.asarray(desc, np.uint8).reshape(n, 32), pre + "cam": np.asarray(cam, f32),
           pre + "sf": FU.SF.astype(f32), pre + "sigma2": SIGMA2, pre + "inv_sigma2": FU.INV_SIGMA2.astype(f32),
           pre + "logsf": np.array([LOGSF], f32)}
    for k, v in more.items():
        if v is not None:
            bag[pre + k] = v
    return bag


def points_bag(points, descs, bad=None, nobs=None):
    """mp_* of FUSE_POINT_DT rows: valid == 0 becomes isBad() unless `bad` says which (a NULL has no object: the list holds -1)."""
    n = len(points)
    return {"mp_pos": points["pos"].astype(f32).reshape(n, 3), "mp_normal": points["normal"].astype(f32).reshape(n, 3),
            "mp_desc": np.asarray(descs, np.uint8).reshape(n, 32),
            "mp_bad": (points["valid"] == 0).astype(np.uint8) if bad is None else np.asarray(bad, np.uint8),
            "mp_min_dist_inv": points["min_dist_inv"].astype(f32), "mp_max_dist_inv": points["max_dist_inv"].astype(f32),
            "mp_max_dist": points["max_dist"].astype(f32), "mp_nobs": np.zeros(n, np.int32) if nobs is None else np.asarray(nobs, np.int32)}


def points_of(arrays, count=None):
    """FUSE_POINT_DT rows and descriptors of the first `count` MapPoints, valid = not bad."""
    n = len(arrays["mp_bad"]) if count is None else count
    pts = np.zeros(n, FU.FUSE_POINT_DT)
    pts["pos"], pts["normal"] = arrays["mp_pos"][:n], arrays["mp_normal"][:n]
    pts["min_dist_inv"], pts["max_dist_inv"], pts["max_dist"] = arrays["mp_min_dist_inv"][:n], arrays["mp_max_dist_inv"][:n], arrays["mp_max_dist"][:n]
    pts["valid"] = arrays["mp_bad"][:n] == 0
    return pts, arrays["mp_desc"][:n]


def concat_points(*bags):
    return {k: np.concatenate([b[k] for b in bags]) for k in bags[0]}


def extra_points(n, bad=None, nobs=None):
    """n MapPoints that only occupy rows: nothing of them is read but isBad() and Observations()."""
    pts = np.zeros(n, FU.FUSE_POINT_DT)
    pts["valid"] = 1
    return points_bag(pts, np.zeros((n, 32), np.uint8), bad=np.zeros(n, np.uint8) if bad is None else bad, nobs=nobs)


def keypoints(x, y, octave, angle=None):
    kp = np.zeros(len(x), KEYPOINT_DT)
    kp["x"], kp["y"], kp["octave"] = x, y, octave
    kp["angle"] = 0 if angle is None else angle
    kp["size"] = 31.0
    return kp


def pose_of_rt(R, t, scale_row=False):
    """Rcw (row major), tcw, Ow = -Rcw.t() * tcw (one gemm, alpha -1) as the stand-in's cv::Mat forms them from a 4 x 4 matrix
    (ORBmatcher.cc:1971-1974, :2329-2331); scale_row: the Sim3 decomposition :483-487 first (the adapter's sim3Pose)."""
    R, t = np.asarray(R, f32).reshape(3, 3), np.asarray(t, f32).reshape(3)
    if scale_row:
        scw = f32(np.sqrt(sum(f64(R[0, j]) * f64(R[0, j]) for j in range(3))))
        inv = 1.0 / f64(scw)
        R, t = (R.astype(f64) * inv).astype(f32), (t.astype(f64) * inv).astype(f32)
    Ow = np.array([f32(-1.0 * (f64(R[0, i]) * f64(t[0]) + f64(R[1, i]) * f64(t[1]) + f64(R[2, i]) * f64(t[2]))) for i in range(3)], f32)
    return np.concatenate([R.reshape(9), t, Ow]).astype(f32)


def mat44(pose):
    T = np.eye(4, dtype=f32)
    T[:3, :3], T[:3, 3] = pose[:9].reshape(3, 3), pose[9:12]
    return T


# ===================================================================================================================== cases
class Case:
    """One scene of one function.  arrays: the inputs (what the fixture stores); calls: the names of its reference calls."""
    fn = None
    exits = ()                                                        # the EXITS tuple of the function's restatement, if it has one

    def __init__(self, name, arrays, calls, tags=()):            # tags: the named edges the case was built for (test_ref_pin_match.py: CONDITIONS)
        self.name, self._arrays, self.calls, self.tags = name, arrays, list(calls), tuple(tags)

    def arrays(self):
        if callable(self._arrays):
            self._arrays = self._arrays()
        return self._arrays

    # per function: bag(arrays, call) -> the driver's case; expected(arrays, result) -> what the fixture says in the restatement's
    # terms; restate(arrays, call, fast, exits, misread) -> the same from the Python restatement; device(fe, arrays, calls)


def _params(*v):
    return np.array(v, f64)


def _fn(name):
    return np.frombuffer(name.encode(), np.uint8).copy()


# --------------------------------------------------------------------------------------------------------------- Fuse (both)
def fuse_arrays(points, descs, kfs, skip, cam=FU.CAM, th=3.0, seed=0):
    """The scene of tests/test_fuse_search_cpu.py as driver tables.  Objects: the list's points, then one per keyframe row that
    holds a map point at entry (about half of them; a tenth of those bad, observations 0-5).  skip[k, i]: IsInKeyFrame for
    Fuse(pKF, vpMapPoints); for Fuse(pKF, Scw, ...) the point is one of the keyframe's own (it sits in a row of its own)."""
    rng = np.random.default_rng(1000 + seed)
    nmp = len(points)
    a = {"th": _params(th), "cam": cam10(cam), "nmp": np.array([nmp], np.int32),
         "skip": np.zeros((len(kfs), nmp), np.uint8) if skip is None else np.asarray(skip, np.uint8)}
    bags, base = [points_bag(points, descs, nobs=rng.integers(0, 6, nmp))], nmp
    for k, kf in enumerate(kfs):
        n = len(kf.x)
        held = rng.random(n) < 0.5
        mp = np.full(n, -1, np.int32)
        mp[held] = base + np.arange(held.sum())
        bags.append(extra_points(int(held.sum()), bad=rng.random(held.sum()) < 0.1, nobs=rng.integers(0, 6, held.sum())))
        base += int(held.sum())
        a.update({"kf%d_%s" % (k, f): v for f, v in zip(KF_FIELDS, (kf.x, kf.y, kf.octave, kf.desc, kf.uright, kf.pose, mp))})
    a.update(concat_points(*bags))
    return a


KF_FIELDS = ("x", "y", "octave", "desc", "uright", "pose", "mp")


def kf_of_arrays(a, k):
    g = lambda f: a["kf%d_%s" % (k, f)]
    return FU.KF(g("x"), g("y"), g("octave"), g("desc"), g("uright"), g("pose"))


def fuse_apply(best_idx, kf_mp, bad, nobs, sim3):
    """What Fuse does with the rows the search found (:1573-1592 / :1715-1729), in list order: the calls on the map, the keyframe's
    rows after them, vpReplacePoint (the Sim3 overload) and the return value."""
    kf_mp, nobs = kf_mp.copy(), nobs.copy()
    ops, replace, nfused = [], np.full(len(best_idx), -1, np.int32), 0
    for i, row in enumerate(best_idx.tolist()):
        if row < 0:
            continue
        held = int(kf_mp[row])
        if held >= 0:
            if not bad[held]:
                if sim3:
                    replace[i] = held
                elif nobs[held] > nobs[i]:
                    ops.append((3, i, held))
                else:
                    ops.append((3, held, i))
        else:
            ops += [(4, i, row), (5, i, row)]
            nobs[i] += 1
            kf_mp[row] = i
        nfused += 1
    return np.array(ops, np.int32).reshape(-1, 3), kf_mp, replace, nfused


def rows_from_ops(ops, nmp):
    """best_idx of every list entry from the recorded calls: GetDescriptor(point) opens a point's search, the GetMapPoint(row)
    before the next one is the row it found."""
    best, cur = np.full(nmp, -1, np.int32), -1
    for op, x, y in ops.tolist():
        if op == 1:
            cur = x
        elif op == 2:
            assert cur >= 0 and best[cur] == -1
            best[cur] = y
    return best


class FuseCase(Case):
    """Fuse(pKF, vpMapPoints, th) per keyframe ("kf<k>") and Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) ("sim3_kf<k>")."""
    fn = "fuse"
    exits = FU.EXITS

    def nkf(self, a):
        return sum(1 for k in a if k.endswith("_pose"))

    def _call(self, call):
        return call.startswith("sim3_"), int(call.split("kf")[1])

    def pose(self, a, call):
        sim3, k = self._call(call)
        p = a["kf%d_pose" % k]
        return pose_of_rt(p[:9], p[9:12], scale_row=True) if sim3 else p

    def skip(self, a, call):
        sim3, k = self._call(call)
        return a["skip"][k]

    def bag(self, a, call):
        sim3, k = self._call(call)
        nmp = int(a["nmp"][0])
        kf = kf_of_arrays(a, k)
        mp = a["kf%d_mp" % k].copy()
        bag = {"fn": _fn("fuse_sim3" if sim3 else "fuse"), "params": _params(0.6, 1, a["th"][0]), "list": np.arange(nmp, dtype=np.int32)}
        bag.update({key: v for key, v in a.items() if key.startswith("mp_")})
        skip = a["skip"][k]
        if sim3:                                                      # a skipped point is the keyframe's own: it gets a row past N
            own = np.nonzero(skip)[0].astype(np.int32)
            bag["Scw"] = mat44(kf.pose)
            pad = lambda v, fill: np.concatenate([v, np.full(len(own), fill, v.dtype)])
            far = f32(-1e6)                                           # outside the grid: no window holds these rows
            t = table_bag("t0_", pad(kf.x, far), pad(kf.y, far), pad(kf.octave, 0), None,
                          np.concatenate([kf.desc, np.zeros((len(own), 32), np.uint8)]), a["cam"], uright=pad(kf.uright, f32(-1)),
                          mp=np.concatenate([mp, own]))
        else:
            ntab = 1
            in_kf = np.zeros((ntab, len(a["mp_bad"])), np.uint8)
            in_kf[0, :nmp] = skip
            bag["mp_in_kf"] = in_kf
            t = table_bag("t0_", kf.x, kf.y, kf.octave, None, kf.desc, a["cam"], uright=kf.uright, mp=mp, R=kf.pose[:9].reshape(3, 3),
                          t=kf.pose[9:12], Ow=kf.pose[12:15])
        bag.update(t)
        return bag

    def expected(self, a, call, res):
        """-> best_idx[nmp], the Replace / AddObservation / AddMapPoint calls, the keyframe's rows, vpReplacePoint, the return."""
        sim3, k = self._call(call)
        nmp, n = int(a["nmp"][0]), len(a["kf%d_x" % k])
        ops = res["ops"].reshape(-1, 3)
        return (rows_from_ops(ops, nmp), ops[ops[:, 0] >= 3], res["kf_mp"][:n], res["replace"] if sim3 else np.full(nmp, -1, np.int32),
                int(res["ret"][0]))

    def restate(self, a, call, fast=False, exits=None, **mis):
        sim3, k = self._call(call)
        nmp = int(a["nmp"][0])
        pts, descs = points_of(a, nmp)
        kf = kf_of_arrays(a, k)._replace(pose=self.pose(a, call))
        if fast:
            best = FU.fuse_search_fast(pts, descs, kf, cam_of(a["cam"]), a["th"][0], not sim3, a["skip"][k])[0]
        else:
            best = FU.fuse_search_scalar(pts, descs, kf, cam_of(a["cam"]), a["th"][0], not sim3, a["skip"][k], exits, **mis)[0]
        return (best,) + fuse_apply(best, a["kf%d_mp" % k], a["mp_bad"], a["mp_nobs"], sim3)

    def device(self, fe, a, calls):
        """device() of every case: {call: (what ONE call over all keyframes / candidates / neighbours of the case gives for this
        call, what a call of its own gives)}, both in expected()'s form.  Here: one batched search per overload, Fuse's second half
        (fuse_apply) on the rows it found."""
        nmp = int(a["nmp"][0])
        pts, descs = points_of(a, nmp)
        out = {}
        for sim3 in (False, True):
            mine = [c for c in calls if self._call(c)[0] == sim3]
            if not mine:
                continue
            ks = [self._call(c)[1] for c in mine]
            kfs = [(keypoints(a["kf%d_x" % k], a["kf%d_y" % k], a["kf%d_octave" % k]), a["kf%d_desc" % k], a["kf%d_uright" % k],
                    self.pose(a, c)) for k, c in zip(ks, mine)]
            skip = np.stack([a["skip"][k] for k in ks])
            bi, _ = fe.fuse_search(pts, descs, kfs, a["cam"][:9], a["th"][0], not sim3, skip, FU.level_ratio())
            one = [fe.fuse_search(pts, descs, [kf], a["cam"][:9], a["th"][0], not sim3, skip[j:j + 1], FU.level_ratio())[0][0]
                   for j, kf in enumerate(kfs)]
            full = lambda best, k: (best,) + fuse_apply(best, a["kf%d_mp" % k], a["mp_bad"], a["mp_nobs"], sim3)
            out.update({c: (full(bi[j], ks[j]), full(one[j], ks[j])) for j, c in enumerate(mine)})
        return out


# ------------------------------------------------------------------------------------- SearchByProjection(pKF, Scw, ...) both
def sim3_arrays(points, descs, kfs, skip, occupied, cam=FU.CAM, th=3.0, ratio=1.0):
    """The scene of tests/test_sim3_projection_cpu.py.  Objects: the list's points, then one per row occupied at entry."""
    nmp = len(points)
    a = {"th": _params(th, ratio), "cam": cam10(cam), "nmp": np.array([nmp], np.int32),
         "skip": np.zeros((len(kfs), nmp), np.uint8) if skip is None else np.asarray(skip, np.uint8)}
    bags, base = [points_bag(points, descs)], nmp
    for k, kf in enumerate(kfs):
        occ = np.zeros(len(kf.x), np.uint8) if occupied is None or occupied[k] is None else np.asarray(occupied[k], np.uint8)
        mp = np.full(len(kf.x), -1, np.int32)
        mp[occ != 0] = base + np.arange(int((occ != 0).sum()))
        bags.append(extra_points(int((occ != 0).sum())))
        base += int((occ != 0).sum())
        a.update({"kf%d_%s" % (k, f): v for f, v in zip(KF_FIELDS, (kf.x, kf.y, kf.octave, kf.desc, kf.uright, kf.pose, mp))})
    a.update(concat_points(*bags))
    return a


class Sim3Case(Case):
    """SearchByProjection(pKF, Scw, vpPoints, vpMatched, th, ratioHamming) ("kf<k>_form0", Pinhole::project) and the overload with
    vpPointsKFs / vpMatchedKF ("kf<k>_form1", the inverse-depth projection), one call per keyframe and form.  vpMatched enters with
    the occupied rows set and, past its N rows, the points this pair leaves out (spAlreadyFound is the set of its entries)."""
    fn = "sim3"
    exits = S3.EXITS

    def _call(self, call):
        k, form = call[2:].split("_form")
        return int(k), int(form)

    def pose(self, a, call):
        p = a["kf%d_pose" % self._call(call)[0]]
        return pose_of_rt(p[:9], p[9:12], scale_row=True)

    def bag(self, a, call):
        k, form = self._call(call)
        nmp = int(a["nmp"][0])
        kf = kf_of_arrays(a, k)
        bag = {"fn": _fn("sim3_kfs" if form else "sim3"), "params": _params(0.6, 1, a["th"][0], a["th"][1]),
               "list": np.arange(nmp, dtype=np.int32), "Scw": mat44(kf.pose),
               "matched": np.concatenate([a["kf%d_mp" % k], np.nonzero(a["skip"][k])[0].astype(np.int32)])}
        if form:
            bag["points_kf"] = np.zeros(nmp, np.int32)                          # every point's keyframe: table 0
        bag.update({key: v for key, v in a.items() if key.startswith("mp_")})
        bag.update(table_bag("t0_", kf.x, kf.y, kf.octave, None, kf.desc, a["cam"], uright=kf.uright))
        return bag

    def expected(self, a, call, res):
        """-> row_point[n], best_idx[nmp], nmatches"""
        k, form = self._call(call)
        nmp, n = int(a["nmp"][0]), len(a["kf%d_x" % k])
        after, before = res["matched"][:n], a["kf%d_mp" % k]
        assert np.array_equal(res["matched"][n:], np.nonzero(a["skip"][k])[0])
        assert ((before < 0) | (after == before)).all()                  # a row occupied at entry keeps its entry
        row_point = np.where(before < 0, after, -1).astype(np.int32)
        best = np.full(nmp, -1, np.int32)
        rows = np.nonzero(row_point >= 0)[0]
        best[row_point[rows]] = rows
        if form:
            assert np.array_equal(res["matched_kf"][:n] >= 0, row_point >= 0)
        return row_point, best, int(res["ret"][0])

    def restate(self, a, call, fast=False, exits=None, **mis):
        k, form = self._call(call)
        pts, descs = points_of(a, int(a["nmp"][0]))
        kf = kf_of_arrays(a, k)._replace(pose=self.pose(a, call))
        occ = (a["kf%d_mp" % k] >= 0).astype(np.uint8)
        if fast:
            return S3.sim3_search_fast(pts, descs, kf, cam_of(a["cam"]), a["th"][0], a["th"][1], form, a["skip"][k], occ)
        return S3.sim3_search_scalar(pts, descs, kf, cam_of(a["cam"]), a["th"][0], a["th"][1], form, a["skip"][k], occ, exits, **mis)

    def device(self, fe, a, calls):
        pts, descs = points_of(a, int(a["nmp"][0]))
        out = {}
        for form in (0, 1):
            mine = [c for c in calls if self._call(c)[1] == form]
            if not mine:
                continue
            ks = [self._call(c)[0] for c in mine]
            pairs = [(keypoints(a["kf%d_x" % k], a["kf%d_y" % k], a["kf%d_octave" % k]), a["kf%d_desc" % k], self.pose(a, c),
                      (a["kf%d_mp" % k] >= 0).astype(np.uint8)) for k, c in zip(ks, mine)]
            skip = np.stack([a["skip"][k] for k in ks])
            rows, bi, nm = fe.search_by_projection_sim3(pts, descs, pairs, a["cam"][:9], a["th"][0], a["th"][1], form, skip, FU.level_ratio())
            for j, c in enumerate(mine):
                r1, b1, n1 = fe.search_by_projection_sim3(pts, descs, pairs[j:j + 1], a["cam"][:9], a["th"][0], a["th"][1], form, skip[j:j + 1],
                                                          FU.level_ratio())
                out[c] = ((rows[j], bi[j], int(nm[j])), (r1[0], b1[0], int(n1[0])))
        return out


# --------------------------------------------------------------------- SearchByProjection(CurrentFrame, pKF, sAlreadyFound, ...)
def reloc_arrays(fr, cands, states, cam=FU.CAM, th=10.0, orb_dist=100, check_ori=True):
    """The scene of tests/test_reloc_projection_cpu.py.  Objects per candidate: its list's points (state 0, NULL, has an object
    that the keyframe does not hold), then one per frame row occupied at entry."""
    a = {"th": _params(th, orb_dist, check_ori), "cam": cam10(cam), "fr_x": fr.x, "fr_y": fr.y, "fr_octave": fr.octave,
         "fr_desc": fr.desc, "fr_angle": fr.angle}
    for k, cd in enumerate(cands):
        nmp = len(cd.points)
        state = np.where(cd.points["valid"] != 0, 3, 1).astype(np.int32) if states is None or states[k] is None else np.asarray(states[k], np.int32)
        occ = np.zeros(len(fr.x), np.uint8) if cd.occupied is None else np.asarray(cd.occupied, np.uint8)
        pb = points_bag(cd.points, cd.descs, bad=state == 1)
        a.update({"c%d_%s" % (k, key): v for key, v in pb.items()})
        a.update({"c%d_state" % k: state, "c%d_angles" % k: np.zeros(nmp, f32) if cd.angles is None else np.asarray(cd.angles, f32),
                  "c%d_pose" % k: cd.pose, "c%d_occupied" % k: occ})
    return a


class RelocCase(Case):
    fn = "reloc"
    exits = RL.EXITS

    def ncand(self, a):
        return sum(1 for k in a if k.endswith("_pose"))

    def cand(self, a, k):
        g = lambda f: a["c%d_%s" % (k, f)]
        pts, descs = points_of({key[len("c%d_" % k):]: v for key, v in a.items() if key.startswith("c%d_mp_" % k)})
        pts["valid"] = g("state") == 3
        p = g("pose")
        return RL.Cand(pts, descs, g("angles"), pose_of_rt(p[:9], p[9:12]), g("occupied"))

    def frame(self, a):
        return RL.FR(a["fr_x"], a["fr_y"], a["fr_octave"], a["fr_desc"], a["fr_angle"])

    def bag(self, a, call):
        k = int(call[1:])
        g = lambda f: a["c%d_%s" % (k, f)]
        nmp, nf = len(g("state")), len(a["fr_x"])
        occ = g("occupied") != 0
        mp = np.full(nf, -1, np.int32)
        mp[occ] = nmp + np.arange(int(occ.sum()))
        bag = {"fn": _fn("reloc"), "params": _params(0.6, a["th"][2], a["th"][0], a["th"][1]),
               "found": np.nonzero(g("state") == 2)[0].astype(np.int32)}
        mps = concat_points({key[len("c%d_" % k):]: v for key, v in a.items() if key.startswith("c%d_mp_" % k)}, extra_points(int(occ.sum())))
        bag.update(mps)
        bag.update(table_bag("t0_", a["fr_x"], a["fr_y"], a["fr_octave"], a["fr_angle"], a["fr_desc"], a["cam"], mp=mp,
                             Tcw=mat44(g("pose"))))
        z = np.zeros(nmp, f32)
        bag.update(table_bag("t1_", z, z, np.zeros(nmp, np.int32), g("angles"), np.zeros((nmp, 32), np.uint8), a["cam"],
                             mp=np.where(g("state") == 0, -1, np.arange(nmp)).astype(np.int32)))
        return bag

    def expected(self, a, call, res):
        """-> row_point[nf], nmatches"""
        k = int(call[1:])
        nmp = len(a["c%d_state" % k])
        after = res["frame_mp"]
        occ = a["c%d_occupied" % k] != 0
        assert (after[occ] >= nmp).all() and (after[~occ] < nmp).all()
        return np.where(occ, -1, after).astype(np.int32), int(res["ret"][0])

    def restate(self, a, call, fast=False, exits=None, **mis):
        k = int(call[1:])
        cd, fr = self.cand(a, k), self.frame(a)
        th, orb_dist, ori = a["th"][0], int(a["th"][1]), bool(a["th"][2])
        if fast:
            r = RL.reloc_search_fast(cd, fr, cam_of(a["cam"]), th, orb_dist, ori)
        else:
            r = RL.reloc_search_scalar(cd, fr, cam_of(a["cam"]), th, orb_dist, ori, exits, a["c%d_state" % k], **mis)
        return r[0], r[2]

    def device(self, fe, a, calls):
        ks = [int(c[1:]) for c in calls]
        fr = self.frame(a)
        kp = keypoints(fr.x, fr.y, fr.octave, fr.angle)
        cands = [tuple(self.cand(a, k)) for k in ks]
        th, orb_dist, ori = a["th"][0], int(a["th"][1]), bool(a["th"][2])
        rows, _, nm = fe.search_by_projection_reloc(cands, kp, fr.desc, a["cam"][:9], th, orb_dist, ori, FU.level_ratio())
        out = {}
        for j, c in enumerate(calls):
            r1, _, n1 = fe.search_by_projection_reloc(cands[j:j + 1], kp, fr.desc, a["cam"][:9], th, orb_dist, ori, FU.level_ratio())
            out[c] = ((rows[j], int(nm[j])), (r1[0], int(n1[0])))
        return out


# ----------------------------------------------------------------------------------------------------------- SearchByBoW (both)
def _bow_table(pre, desc, angle, node, cam=FU.CAM, mp=None):
    n = len(node)
    z = np.zeros(n, f32)
    return table_bag(pre, z, z, np.zeros(n, np.int32), angle, desc, cam10(cam), node=np.asarray(node, np.int32), mp=mp)


def _bow_objects(valid, base, rng_bit=0):
    """Row i holds object base + i; an invalid row alternates between NULL and a bad point.  -> mp[n], bad[n]"""
    valid = np.asarray(valid) != 0
    idx = np.arange(len(valid))
    null = ~valid & ((idx + rng_bit) % 2 == 0)
    return np.where(null, -1, base + idx).astype(np.int32), (~valid).astype(np.uint8)


def bow_arrays(kfs, frame, nnratio=0.75, check_ori=True):
    """kfs: [(desc, angle, node, valid)], frame: (desc, angle, node) as tests/test_bow_search_cpu.py has them."""
    a = {"th": _params(nnratio, check_ori), "f_desc": np.asarray(frame[0], np.uint8).reshape(-1, 32), "f_angle": np.asarray(frame[1], f32),
         "f_node": np.asarray(frame[2], np.int32)}
    for k, (d, ang, node, valid) in enumerate(kfs):
        a.update({"kf%d_desc" % k: np.asarray(d, np.uint8).reshape(-1, 32), "kf%d_angle" % k: np.asarray(ang, f32),
                  "kf%d_node" % k: np.asarray(node, np.int32), "kf%d_valid" % k: np.asarray(valid, np.uint8)})
    return a


class BowCase(Case):
    """SearchByBoW(pKF, F, vpMapPointMatches), one call per keyframe ("kf<k>").  The map point of keyframe row i is object i."""
    fn = "bow"

    def kf(self, a, k):
        return tuple(a["kf%d_%s" % (k, f)] for f in ("desc", "angle", "node", "valid"))

    def bag(self, a, call):
        d, ang, node, valid = self.kf(a, int(call[2:]))
        mp, bad = _bow_objects(valid, 0)
        pts = np.zeros(len(node), FU.FUSE_POINT_DT)
        bag = {"fn": _fn("bow"), "params": _params(a["th"][0], a["th"][1])}
        if len(node):
            bag.update(points_bag(pts, np.zeros((len(node), 32), np.uint8), bad=bad))
        bag.update(_bow_table("t0_", d, ang, node, mp=mp))
        bag.update(_bow_table("t1_", a["f_desc"], a["f_angle"], a["f_node"]))
        return bag

    def expected(self, a, call, res):
        """-> matches[nf] (the keyframe's row), nmatches"""
        return res["matches"].astype(np.int32), int(res["ret"][0])

    def restate(self, a, call, fast=False, exits=None, **mis):
        fn = BW.search_by_bow_fast if fast else BW.search_by_bow
        return fn(*self.kf(a, int(call[2:])), a["f_desc"], a["f_angle"], a["f_node"], a["th"][0], bool(a["th"][1]), **mis)

    def device(self, fe, a, calls):
        kfs = [self.kf(a, int(c[2:])) for c in calls]
        m, n = fe.search_by_bow(a["f_desc"], a["f_angle"], a["f_node"], kfs, a["th"][0], bool(a["th"][1]))
        out = {}
        for j, c in enumerate(calls):
            m1, n1 = fe.search_by_bow(a["f_desc"], a["f_angle"], a["f_node"], kfs[j:j + 1], a["th"][0], bool(a["th"][1]))
            out[c] = ((m[j], int(n[j])), (m1[0], int(n1[0])))
        return out

    def oracle(self, po, a, call):
        return None


def bow_kf_arrays(kf1, kfs, nnratio=0.75, check_ori=True):
    a = bow_arrays(kfs, kf1[:3], nnratio, check_ori)
    a["f_valid"] = np.asarray(kf1[3], np.uint8)
    return a


class BowKfCase(BowCase):
    """SearchByBoW(pKF1, pKF2, vpMatches12), one call per pKF2 ("kf<k>"); pKF1 is the table "f".  Objects: pKF1's rows, then
    pKF2's."""
    fn = "bow_kf"

    def bag(self, a, call):
        d, ang, node, valid = self.kf(a, int(call[2:]))
        n1, n2 = len(a["f_node"]), len(node)
        mp1, bad1 = _bow_objects(a["f_valid"], 0)
        mp2, bad2 = _bow_objects(valid, n1, 1)
        bag = {"fn": _fn("bow_kf"), "params": _params(a["th"][0], a["th"][1])}
        if n1 + n2:
            bag.update(points_bag(np.zeros(n1 + n2, FU.FUSE_POINT_DT), np.zeros((n1 + n2, 32), np.uint8), bad=np.concatenate([bad1, bad2])))
        bag.update(_bow_table("t0_", a["f_desc"], a["f_angle"], a["f_node"], mp=mp1))
        bag.update(_bow_table("t1_", d, ang, node, mp=mp2))
        return bag

    def expected(self, a, call, res):
        """-> matches12[n1] (pKF2's row), nmatches"""
        n1 = len(a["f_node"])
        m = res["matches"].astype(np.int32)
        assert len(m) == n1 and ((m < 0) | (m >= n1)).all()
        return np.where(m >= 0, m - n1, -1).astype(np.int32), int(res["ret"][0])

    def restate(self, a, call, fast=False, exits=None, **mis):
        fn = BK.search_by_bow_kf_fast if fast else BK.search_by_bow_kf
        return fn(a["f_desc"], a["f_angle"], a["f_node"], a["f_valid"], *self.kf(a, int(call[2:])), a["th"][0], bool(a["th"][1]), **mis)

    def device(self, fe, a, calls):
        kfs = [self.kf(a, int(c[2:])) for c in calls]
        one = (a["f_desc"], a["f_angle"], a["f_node"], a["f_valid"])
        m, n = fe.search_by_bow_kf(*one, kfs, a["th"][0], bool(a["th"][1]))
        out = {}
        for j, c in enumerate(calls):
            m1, n1 = fe.search_by_bow_kf(*one, kfs[j:j + 1], a["th"][0], bool(a["th"][1]))
            out[c] = ((m[j], int(n[j])), (m1[0], int(n1[0])))
        return out


# ------------------------------------------------------------------------------------------------- SearchForInitialization
def _t(a, pre):
    return IN.T(a[pre + "x"], a[pre + "y"], a[pre + "octave"], a[pre + "desc"], a[pre + "angle"])


def init_arrays(t1, frames, prev=None, bounds=IN.BOUNDS, window=100, nnratio=0.9, check_ori=True):
    a = {"th": _params(nnratio, check_ori, window), "bounds": np.array(bounds, f32),
         "prev": IN.points_of(t1) if prev is None else np.asarray(prev, f32).reshape(-1, 2)}
    for pre, t in [("f0_", t1)] + [("f%d_" % (k + 1), t) for k, t in enumerate(frames)]:
        a.update({pre + f: v for f, v in zip(IN.T._fields, t)})
    return a


class InitCase(Case):
    """SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize): ONE call "chain" of the program, which searches the
    frames 1, 2, ... in turn and carries vbPrevMatched, as Tracking does."""
    fn = "init"
    exits = IN.EXITS

    def nframes(self, a):
        return sum(1 for k in a if k.endswith("_x")) - 1

    def bag(self, a, call):
        b = a["bounds"]
        cam = np.array([1, 1, 0, 0, 0, b[0], b[1], b[2], b[3], 0], f32)
        bag = {"fn": _fn("init"), "params": _params(a["th"][0], a["th"][1], a["th"][2]), "prev": a["prev"]}
        for k in range(self.nframes(a) + 1):
            t = _t(a, "f%d_" % k)
            bag.update(table_bag("t%d_" % k, t.x, t.y, t.octave, t.angle, t.desc, cam))
        return bag

    def expected(self, a, call, res):
        """-> [(matches12, nmatches, vbPrevMatched after) per frame]"""
        return [(res["matches12"][k], int(res["rets"][k]), res["prev"][k]) for k in range(len(res["rets"]))]

    def restate(self, a, call, fast=False, exits=None, **mis):
        fn = IN.init_search_fast if fast else IN.init_search_scalar
        kw = dict(bounds=tuple(a["bounds"].tolist()), window=int(a["th"][2]), nnratio=a["th"][0], check_ori=bool(a["th"][1]))
        if not fast:
            kw.update(exits=exits, **mis)
        prev, out = a["prev"], []
        for k in range(1, self.nframes(a) + 1):
            _, m12, nm, prev = fn(_t(a, "f0_"), _t(a, "f%d_" % k), prev, **kw)
            out.append((m12, nm, prev))
        return out

    def device(self, fe, a, calls):
        t1 = _t(a, "f0_")
        prev, out = a["prev"], []
        for k in range(1, self.nframes(a) + 1):
            t2 = _t(a, "f%d_" % k)
            nm, m12, _, prev = fe.search_for_initialization(IN.keypoints(t1), t1.desc, prev, IN.keypoints(t2), t2.desc,
                                                            tuple(a["bounds"].tolist()), int(a["th"][2]), a["th"][0], bool(a["th"][1]))
            out.append((m12, nm, prev))
        return {"chain": (out, out)}


# -------------------------------------------------------------------------------------------------- SearchForTriangulation
def tri_geometry(R1w, t1w, Cw, K1, R2w, t2w, K2):
    """F12 and the epipole as the stand-in's cv::Mat forms them from ORBmatcher.cc:972-992 and Pinhole.cpp:124-127: the adapter's
    pli_detail::triangulationGeometry (pli_slam_amd/adapters/orbslam_adapters.hpp), line by line."""
    def gemm(A, ta, alpha, B, tb, C=None):
        A, B = (A.T if ta else A).astype(f64), (B.T if tb else B).astype(f64)
        out = np.zeros((A.shape[0], B.shape[1]), f32)
        for i in range(A.shape[0]):
            for j in range(B.shape[1]):
                d = 0.0
                for k in range(A.shape[1]):
                    d += A[i, k] * B[k, j]
                out[i, j] = f32(alpha * d + (f64(C[i, j]) if C is not None else 0.0))
        return out

    def inv3(S):
        S = S.astype(f64).reshape(9)
        det = S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6]) + S[2] * (S[3] * S[7] - S[4] * S[6])
        if det == 0.0:
            return np.zeros((3, 3), f32)
        d = 1.0 / det
        co = [S[4] * S[8] - S[5] * S[7], S[2] * S[7] - S[1] * S[8], S[1] * S[5] - S[2] * S[4], S[5] * S[6] - S[3] * S[8],
              S[0] * S[8] - S[2] * S[6], S[2] * S[3] - S[0] * S[5], S[3] * S[7] - S[4] * S[6], S[1] * S[6] - S[0] * S[7],
              S[0] * S[4] - S[1] * S[3]]
        return np.array([f32(c * d) for c in co], f32).reshape(3, 3)

    R1w, R2w = np.asarray(R1w, f32).reshape(3, 3), np.asarray(R2w, f32).reshape(3, 3)
    t1w, t2w, Cw = (np.asarray(v, f32).reshape(3, 1) for v in (t1w, t2w, Cw))
    K1, K2 = np.asarray(K1, f32), np.asarray(K2, f32)
    C2 = gemm(R2w, False, 1.0, Cw, False, t2w).reshape(3)
    with np.errstate(all="ignore"):
        ep = np.array([f32(f32(f32(K2[0] * C2[0]) / C2[2]) + K2[2]), f32(f32(f32(K2[1] * C2[1]) / C2[2]) + K2[3])], f32)
    R12 = gemm(R1w, False, 1.0, R2w, True)
    t12 = gemm(gemm(R1w, False, -1.0, R2w, True), False, 1.0, t2w, False, t1w).reshape(3)
    z = f32(0)
    t12x = np.array([[z, -t12[2], t12[1]], [t12[2], z, -t12[0]], [-t12[1], t12[0], z]], f32)
    K1t = np.array([[K1[0], 0, 0], [0, K1[1], 0], [K1[2], K1[3], 1]], f32)
    K2m = np.array([[K2[0], 0, K2[2]], [0, K2[1], K2[3]], [0, 0, 1]], f32)
    F12 = gemm(gemm(gemm(inv3(K1t), False, 1.0, t12x, False), False, 1.0, R12, False), False, 1.0, inv3(K2m), False)
    return F12, ep


TRI_FIELDS = TR.Table._fields
TRI_SETTINGS = [(os_, co, ori) for os_ in (0, 1) for co in (0, 1) for ori in (0, 1)]


def tri_arrays(t1, nbrs, poses, K=TR.K_EUROC, settings=TRI_SETTINGS):
    """t1, [t2], [(R1w, t1w, R2w, t2w)] of two_view_case; the keyframes' stored camera centre is make_pose's."""
    a = {"K": np.array(K, f32), "settings": np.array(settings, np.int32).reshape(-1, 3)}
    a.update({"t1_" + f: v for f, v in zip(TRI_FIELDS, t1)})
    for k, (t2, (R1w, t1w, R2w, t2w)) in enumerate(zip(nbrs, poses)):
        a.update({"n%d_%s" % (k, f): v for f, v in zip(TRI_FIELDS, t2)})
        a["n%d_pose1" % k], a["n%d_pose2" % k] = FU.make_pose(R1w, t1w), FU.make_pose(R2w, t2w)
    return a


class TriCase(Case):
    """SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo, bCoarse), one call per neighbour and setting
    ("n<k>_s<onlyStereo><coarse><checkOrientation>").  The reference forms F12 and the epipole itself, from the poses."""
    fn = "tri"
    exits = TR.EXITS

    def _call(self, call):
        k, s = call[1:].split("_s")
        return int(k), tuple(int(c) for c in s)

    def tables(self, a, k):
        return TR.Table(*[a["t1_" + f] for f in TRI_FIELDS]), TR.Table(*[a["n%d_%s" % (k, f)] for f in TRI_FIELDS])

    def geometry(self, a, k):
        p1, p2 = a["n%d_pose1" % k], a["n%d_pose2" % k]
        return tri_geometry(p1[:9], p1[9:12], p1[12:15], a["K"], p2[:9], p2[9:12], a["K"])

    def bag(self, a, call):
        k, (os_, co, ori) = self._call(call)
        K = a["K"]
        cam = np.array([K[0], K[1], K[2], K[3], 0, 0, 752, 0, 480, 0], f32)
        bag = {"fn": _fn("tri"), "params": _params(0.6, ori, os_, co)}
        base, bags = 0, []
        for pre, t, pose in zip(("t0_", "t1_"), self.tables(a, k), (a["n%d_pose1" % k], a["n%d_pose2" % k])):
            n = len(t.node)
            mp = np.where(t.has_mp != 0, base + np.arange(n), -1).astype(np.int32)
            base += n
            bags.append(extra_points(n))
            bag.update(table_bag(pre, t.x, t.y, t.octave, t.angle, t.desc, cam, node=t.node, mp=mp,
                                 uright=np.where(t.stereo != 0, f32(1.0), f32(-1.0)).astype(f32), R=pose[:9].reshape(3, 3), t=pose[9:12],
                                 Ow=pose[12:15]))
        bag.update(concat_points(*bags))
        return bag

    def expected(self, a, call, res):
        """-> vMatches12[n1] (from vMatchedPairs, which lists them by idx1), nmatches"""
        m = np.full(len(a["t1_node"]), -1, np.int32)
        pairs = res["pairs"].reshape(-1, 2)
        assert (np.diff(pairs[:, 0]) > 0).all()
        m[pairs[:, 0]] = pairs[:, 1]
        return m, int(res["ret"][0])

    def restate(self, a, call, fast=False, exits=None, **mis):
        k, (os_, co, ori) = self._call(call)
        t1, t2 = self.tables(a, k)
        F12, ep = self.geometry(a, k)
        if fast:
            return TR.search_for_triangulation_fast(t1, t2, F12, ep, bool(os_), bool(co), bool(ori))
        return TR.search_for_triangulation(t1, t2, F12, ep, bool(os_), bool(co), bool(ori), exits, **mis)

    def device(self, fe, a, calls):
        out = {}
        pack = lambda t: (keypoints(t.x, t.y, t.octave, t.angle), t.desc, t.node, t.has_mp, t.stereo)
        for s in sorted({self._call(c)[1] for c in calls}):
            mine = [c for c in calls if self._call(c)[1] == s]
            ks = [self._call(c)[0] for c in mine]
            t1 = self.tables(a, ks[0])[0]
            kfs = [pack(self.tables(a, k)[1]) + self.geometry(a, k) for k in ks]
            m, n = fe.search_for_triangulation(pack(t1), kfs, bool(s[0]), bool(s[1]), bool(s[2]))
            for j, c in enumerate(mine):
                m1, n1 = fe.search_for_triangulation(pack(t1), kfs[j:j + 1], bool(s[0]), bool(s[1]), bool(s[2]))
                out[c] = ((m[j], int(n[j])), (m1[0], int(n1[0])))
        return out


# ----------------------------------------------------- SearchByProjection(F, vpMapPoints, ...) and (CurrentFrame, LastFrame, ...)
IDENTITY_CAM = np.array([1, 1, 0, 0, 5, 0, 640, 0, 480, 0], f32)          # u = x / z exactly; ur = u - 5 / z


def _cur_table(a, mb=None):
    """The current frame's table for the driver; cur_occ: 0 = NULL, 1 = a map point with observations, 2 = one without.  The
    objects of the rows follow the `base` list points."""
    base = len(a["mp_bad"])
    occ = a["cur_occ"]
    mp = np.full(len(occ), -1, np.int32)
    mp[occ != 0] = base + np.arange(int((occ != 0).sum()))
    extra = extra_points(int((occ != 0).sum()), nobs=np.where(occ[occ != 0] == 1, 3, 0))
    cam = a["cam"].copy()
    return mp, extra, table_bag("t0_", a["cur_x"], a["cur_y"], a["cur_octave"], a["cur_angle"], a["cur_desc"], cam, uright=a["cur_uright"],
                                mp=mp, **({"Tcw": a["cur_Tcw"]} if "cur_Tcw" in a else {}))


def rows_after(raw, best, nrows, no_obs=None):
    """The frame's rows once every match is written (in list order, a later one over an earlier) and the rotation filter has set the
    rows of ITS entries back to NULL, whoever holds them by then (:2163-2173)."""
    rows = np.full(nrows, -1, np.int32)
    for i in np.nonzero(raw >= 0)[0]:
        rows[raw[i]] = i
    for i in np.nonzero((raw >= 0) & (best < 0))[0]:
        rows[raw[i]] = -1
    return rows


class _ProjCase(Case):
    def kp(self, a):
        return keypoints(a["cur_x"], a["cur_y"], a["cur_octave"], a["cur_angle"])

    def bounds(self, a):
        return tuple(float(v) for v in a["cam"][5:9])

    def expected(self, a, call, res):
        """-> the rows of the current frame that hold a list point after the call (-1: none, or what they held before), the return"""
        nq = len(self.queries(a)[0])
        rows = res["frame_mp"]
        return np.where(rows < nq, rows, -1).astype(np.int32), int(res["ret"][0])

    def count(self, exits, labels):
        if exits is not None:
            for e in labels:
                exits[e[0]] += 1
                for tag in e[1:]:
                    exits["tag:" + tag] += 1


def local_arrays(kp, desc, ur, occ, track, qdesc, bad, bounds, th=1.0, far=False, th_far=50.0, nnratio=0.8):
    """track[nq, 8]: mbTrackInView, mTrackProjX, mTrackProjY, mTrackProjXR, mTrackDepth, mnTrackScaleLevel, mTrackViewCos, 0."""
    nq = len(track)
    pts = np.zeros(nq, FU.FUSE_POINT_DT)
    cam = IDENTITY_CAM.copy()
    cam[5:9] = bounds
    a = {"th": _params(th, far, th_far, nnratio), "cam": cam, "cur_x": kp["x"], "cur_y": kp["y"], "cur_octave": kp["octave"],
         "cur_angle": kp["angle"], "cur_desc": desc, "cur_uright": np.asarray(ur, f32), "cur_occ": np.asarray(occ, np.uint8),
         "mp_track": np.asarray(track, f32).reshape(nq, 8)}
    a.update(points_bag(pts, qdesc, bad=bad, nobs=np.ones(nq, np.int32)))
    return a


class LocalCase(_ProjCase):
    """SearchByProjection(F, vpMapPoints, th, bFarPoints, thFarPoints): one call."""
    fn = "local"
    exits = ("invalid", "no_features_in_area", "no_candidate", "distance_above_TH_HIGH", "matched", "ratio_test_failed_same_level")

    def queries(self, a):
        """:50-73: who takes part, the radius from the viewing cosine and th, the level window [level - 1, level]."""
        t = a["mp_track"]
        th, far, th_far = f32(a["th"][0]), bool(a["th"][1]), f32(a["th"][2])
        q = np.zeros(len(t), HM.PROJ_QUERY_DT)
        for i, (inview, px, py, pxr, depth, level, cos, _) in enumerate(t):
            r = f32(2.5) if float(cos) > 0.998 else f32(4.0)
            if float(th) != 1.0:
                r = f32(r * th)
            level = int(level)
            q[i] = (px, py, f32(r * FU.SF[level]), pxr, level - 1, level, 0, int(inview != 0 and not (far and depth > th_far) and not a["mp_bad"][i]))
        return q, a["mp_desc"]

    def bag(self, a, call):
        mp, extra, tab = _cur_table(a)
        bag = {"fn": _fn("local"), "params": _params(a["th"][3], 1, a["th"][0], a["th"][1], a["th"][2]),
               "list": np.arange(len(a["mp_track"]), dtype=np.int32)}
        pts = {k: v for k, v in a.items() if k.startswith("mp_") and k != "mp_track"}
        bag.update(concat_points(pts, extra))
        bag["mp_track"] = np.concatenate([a["mp_track"], np.zeros((len(extra["mp_bad"]), 8), f32)])
        bag.update(tab)
        return bag

    def restate(self, a, call, fast=False, exits=None, **mis):
        q, qd = self.queries(a)
        n, best, labels = HM.search_local_map(q, qd, self.kp(a), a["cur_desc"], a["cur_uright"], a["cur_occ"] == 1, self.bounds(a),
                                              a["th"][3], **mis)
        self.count(exits, labels)
        return rows_after(best, best, len(a["cur_x"])), n

    def device(self, fe, a, calls):
        q, qd = self.queries(a)
        n, best = fe.search_local_map(q, qd, self.kp(a), a["cur_desc"], a["cur_uright"], self.bounds(a), a["th"][3], (a["cur_occ"] == 1).astype(np.uint8))
        r = (rows_after(best, best, len(a["cur_x"])), n)
        return {"call": (r, r)}


def frame_arrays(kp, desc, ur, occ, pos, qdesc, nobs, last_octave, last_angle, last_held, last_outlier, cur_pose, last_pose, cam,
                 th=15.0, mono=False, check_ori=True):
    """Row i of the last frame holds list point i when last_held[i].  cam: 10 floats (fx fy cx cy bf minX maxX minY maxY mb)."""
    nq = len(pos)
    pts = np.zeros(nq, FU.FUSE_POINT_DT)
    pts["pos"] = pos
    a = {"th": _params(th, mono, check_ori), "cam": np.asarray(cam, f32), "cur_x": kp["x"], "cur_y": kp["y"], "cur_octave": kp["octave"],
         "cur_angle": kp["angle"], "cur_desc": desc, "cur_uright": np.asarray(ur, f32), "cur_occ": np.asarray(occ, np.uint8),
         "cur_Tcw": mat44(cur_pose), "last_Tcw": mat44(last_pose), "last_octave": np.asarray(last_octave, np.int32),
         "last_angle": np.asarray(last_angle, f32), "last_held": np.asarray(last_held, np.uint8), "last_outlier": np.asarray(last_outlier, np.uint8)}
    a.update(points_bag(pts, qdesc, bad=np.zeros(nq, np.uint8), nobs=nobs))
    return a


class FrameCase(_ProjCase):
    """SearchByProjection(CurrentFrame, LastFrame, th, bMono): one call."""
    fn = "frame"
    exits = ("invalid", "outside_bounds", "no_features_in_area", "no_candidate", "distance_above_TH_HIGH", "matched",
             "matched_then_rotation_filtered")

    def queries(self, a, inverse_depth=False):
        """:1971-2022: the projection of every point the last frame holds (Pinhole::project, :2002), the window from its octave and the
        direction of motion.  inverse_depth: the projection of the OTHER overload (the one with match12, :2222-2223: fx*xc*invzc + cx),
        a misreading here."""
        cam, th, mono = a["cam"], f32(a["th"][0]), bool(a["th"][1])
        Tc, Tl = a["cur_Tcw"], a["last_Tcw"]
        Rcw, tcw = Tc[:3, :3], Tc[:3, 3]
        twc = pose_of_rt(Rcw, tcw)[12:15]
        tlc_z = FU.gemm_row(Tl[2, :3], twc, Tl[2, 3])
        forward, backward = bool(tlc_z > cam[9]) and not mono, bool(-tlc_z > cam[9]) and not mono
        n = len(a["last_octave"])
        q = np.zeros(n, HM.PROJ_QUERY_DT)
        with np.errstate(all="ignore"):
            for i in range(n):
                if not a["last_held"][i] or a["last_outlier"][i]:
                    continue
                p = a["mp_pos"][i]
                x, y, z = (FU.gemm_row(Rcw[r], p, tcw[r]) for r in range(3))
                invz = f32(1.0 / f64(z))
                if invz < 0:
                    continue
                u = f32(f32(f32(cam[0] * x) / z) + cam[2])
                v = f32(f32(f32(cam[1] * y) / z) + cam[3])
                if inverse_depth:
                    u, v = f32(f32(f32(cam[0] * x) * invz) + cam[2]), f32(f32(f32(cam[1] * y) * invz) + cam[3])
                o = int(a["last_octave"][i])
                lo, hi = (o, -1) if forward else (0, o) if backward else (o - 1, o + 1)
                q[i] = (u, v, f32(th * FU.SF[o]), f32(u - f32(cam[4] * invz)), lo, hi, a["last_angle"][i], 1 if a["mp_nobs"][i] > 0 else 3)
        return q, a["mp_desc"]

    def bag(self, a, call):
        nq = len(a["last_octave"])
        mp, extra, tab = _cur_table(a)
        bag = {"fn": _fn("frame"), "params": _params(0.9, a["th"][2], a["th"][0], a["th"][1])}
        bag.update(concat_points({k: v for k, v in a.items() if k.startswith("mp_")}, extra))
        bag.update(tab)
        z = np.zeros(nq, f32)
        bag.update(table_bag("t1_", z, z, a["last_octave"], a["last_angle"], np.zeros((nq, 32), np.uint8), a["cam"],
                             mp=np.where(a["last_held"] != 0, np.arange(nq), -1).astype(np.int32), outlier=a["last_outlier"], Tcw=a["last_Tcw"]))
        return bag

    def restate(self, a, call, fast=False, exits=None, inverse_depth=False, **mis):
        q, qd = self.queries(a, inverse_depth)
        n, best, raw, labels, _ = HM.search_by_projection(q, qd, self.kp(a), a["cur_desc"], a["cur_uright"], self.bounds(a), bool(a["th"][2]),
                                                          a["cur_occ"] == 1, **mis)
        self.count(exits, labels)
        return rows_after(raw, best, len(a["cur_x"])), n

    def device(self, fe, a, calls):
        q, qd = self.queries(a)
        n, best, raw = fe.search_by_projection(q, qd, self.kp(a), a["cur_desc"], a["cur_uright"], self.bounds(a), bool(a["th"][2]),
                                               (a["cur_occ"] == 1).astype(np.uint8), with_raw=True)
        r = (rows_after(raw, best, len(a["cur_x"])), n)
        return {"call": (r, r)}


# =================================================================================================================== the corpus
def _fuse_seeded(seed, nkf, nmp, nfeat):
    def make():
        pts, descs, kfs, skip = FU.fuse_case(np.random.default_rng(seed), nkf, nmp, nfeat)
        return fuse_arrays(pts, descs, kfs, skip, th=3.0 if seed % 2 else 4.0, seed=seed)
    return make


def _fuse_hand():
    """The known-answer tables of tests/test_fuse_search_cpu.py, one keyframe each (identity pose, so the Sim3 decomposition
    returns the pose bit for bit): kf0 equal distances in two cells (the earlier in visiting order wins) and the chi-square gates
    at both bounds; kf1 a distance of exactly TH_LOW and TH_LOW + 1; kf2 a projection exactly on mnMaxX (outside) and one float
    below it."""
    d = np.arange(32, dtype=np.uint8)
    rng = np.random.default_rng(40)
    P = [FU.point_at_pixel(100.0, 100.0), FU.point_at_pixel(300.0, 100.0), FU.point_at_pixel(500.0, 100.0), FU.point_at_pixel(300.0, 300.0)]
    edge, x = FU.point_at_pixel(300.0, 200.0), f32((752.0 - float(FU.CAM.cx)) * 4.0 / float(FU.CAM.fx))
    for _ in range(400):                                             # the float x whose projection rounds to 752 exactly
        u = f32(f32(f32(FU.CAM.fx * x) / f32(4.0)) + FU.CAM.cx)
        if u == f32(752.0):
            break
        x = np.nextafter(x, f32(np.inf) if u < f32(752.0) else f32(-np.inf))
    assert u == f32(752.0)
    edge["pos"][0] = [x, 0.0, 4.0]
    below = edge.copy()
    while True:
        below["pos"][0, 0] = np.nextafter(below["pos"][0, 0], f32(-np.inf))
        if f32(f32(f32(FU.CAM.fx * below["pos"][0, 0]) / f32(4.0)) + FU.CAM.cx) < f32(752.0):
            break
    for p in (edge, below):                                          # ratio 3.2: level 7, a window of 3 * 3.58 px that reaches into the grid
        p["max_dist"] = 3.2 * np.linalg.norm(p["pos"][0].astype(f64))
    pts = np.concatenate(P + [edge, below])
    descs = np.stack([d] * len(pts))
    near = lambda n: FU.flip_bits(rng, d, n)
    e = near(7)
    # kf0: twins at equal distance on both sides of a cell boundary (cell width 11.75 px: x = 99 and 101.5 lie in cells 8 and 9),
    # listed in the order that the index alone would get wrong; chi-square: 5.99 and 7.8 at level 0 are 2.447^2 and 2.793^2
    kf0 = FU.kf_of([101.5, 99.0, 302.44, 302.46, 500.0, 500.0], [100.0, 100.0, 100.0, 100.0, 102.0, 102.0], [e, e, near(3), near(5), near(3), near(5)],
                   uright=[-1, -1, -1, -1, f32(500.0) - FU.CAM.bf / f32(4.0) + f32(1.9), f32(500.0) - FU.CAM.bf / f32(4.0) + f32(2.0)])
    kf1 = FU.kf_of([100.0, 300.0, 500.0, 300.0], [100.0, 100.0, 100.0, 300.0], [near(50), near(51), near(49), near(0)])
    kf2 = FU.kf_of([744.0, 745.0], [float(FU.CAM.cy)] * 2, [near(2), near(4)], octaves=[7, 7])      # (x >= 746.2 is off the grid)
    return fuse_arrays(pts, descs, [kf0, kf1, kf2], None, th=3.0, seed=40)


def _sim3_seeded(seed, npair, nmp, nfeat, th, ratio):
    def make():
        pts, descs, kfs, skip, occ = S3.sim3_case(np.random.default_rng(seed), npair, nmp, nfeat)
        return sim3_arrays(pts, descs, kfs, skip, occ, th=th, ratio=ratio)
    return make


def _edge_points(form):
    """Two points in front of the identity camera at z = 4 and level 7 (a window of 3 * 3.58 px that reaches into the grid): the first
    projects to u = mnMaxX = 752 exactly under the given projection form (the float x is stepped until it does), the second one float
    x below it."""
    cam, z, target = FU.CAM, f32(4.0), f32(752.0)
    proj = lambda x: S3.project_uv(f32(x), f32(0.0), z, cam, form)[0]
    x = f32((752.0 - float(cam.cx)) * 4.0 / float(cam.fx))
    for _ in range(400):
        u = proj(x)
        if u == target:
            break
        x = np.nextafter(x, f32(np.inf) if u < target else f32(-np.inf))
    assert proj(x) == target
    below = x
    while not proj(below) < target:
        below = np.nextafter(below, f32(-np.inf))
    pts = []
    for xx in (x, below):
        p = FU.point_at_pixel(300.0, 200.0)
        p["pos"][0] = [xx, 0.0, z]
        p["max_dist"] = 3.2 * np.linalg.norm(p["pos"][0].astype(f64))
        pts.append(p)
    return pts


def _sim3_edge():
    """KeyFrame::IsInImage at mnMaxX (:522 / :639): for each projection form a point exactly on it (outside) and one a float below
    (inside), each with a keypoint of its own descriptor in reach (x >= 746.2 is off the grid)."""
    rng = np.random.default_rng(41)
    pts = np.concatenate(_edge_points(0) + _edge_points(1))
    descs = rng.integers(0, 256, (4, 32), dtype=np.uint8)
    kf = FU.kf_of([744.0, 744.5, 745.0, 745.5], [float(FU.CAM.cy)] * 4, descs.copy(), octaves=[7] * 4)
    return sim3_arrays(pts, descs, [kf], None, None)


def _sim3_hand(which):
    def make():
        if which == "reversal":
            pts, descs, kf = S3.reversal_case()
            return sim3_arrays(np.concatenate([pts, pts[::-1]]), np.concatenate([descs, descs[::-1]]), [kf, kf],
                               np.array([[0, 0, 0, 1, 1, 1], [1, 1, 1, 0, 0, 0]], np.uint8), None)
        if which == "boundary":
            pts, descs, kf, _ = S3.boundary_case()
            return sim3_arrays(pts, descs, [kf], None, None)
        if which in ("thresholds", "thresholds_ratio15"):          # distances around TH_LOW * ratioHamming itself: 50, and 75.0f
            rng = np.random.default_rng(7)
            d = rng.integers(0, 256, 32, dtype=np.uint8)
            P = FU.point_at_pixel(300.0, 200.0)
            ratio, around = (1.0, 50) if which == "thresholds" else (1.5, 75)
            kfs = [FU.kf_of([300], [200], [FU.flip_bits(rng, d, n)]) for n in (around - 1, around, around + 1, around + 2)]
            return sim3_arrays(P, d[None], kfs, None, None, ratio=ratio)
        if which == "edge":
            return _sim3_edge()
        name = which
        pts, descs, kf, kw, _, _ = S3.contention_cases()[name]
        return sim3_arrays(pts, descs, [kf], None if "skip" not in kw else kw["skip"][None], [kw.get("occupied")])
    return make


def _reloc_seeded(seed, ncand, nmp, nfeat, th, orb_dist):
    def make():
        fr, cands, states = RL.reloc_case(np.random.default_rng(seed), ncand, nmp, nfeat)
        return reloc_arrays(fr, cands, states, th=th, orb_dist=orb_dist)
    return make


def _reloc_hand(which):
    def make():
        if which == "behind":
            cd, fr = RL.behind_case()
        elif which == "edge":
            cd, fr, _ = RL.edge_case()
        elif which == "filtered_row":
            cd, fr = RL.filtered_row_case()[:2]
        elif which == "tie":                                        # equal distances in two cells, listed against the walking order
            d = np.arange(32, dtype=np.uint8)
            e = FU.flip_bits(np.random.default_rng(8), d, 6)
            cd, fr = RL.cand_of(FU.point_at_pixel(300.0, 200.0), [d]), RL.frame_of([305.5, 299.0], [200.0, 200.0], [e, e])
        elif which == "reversal":
            pts, descs, fr = RL.reversal_case()
            return reloc_arrays(fr, [RL.cand_of(pts, descs), RL.cand_of(pts[::-1].copy(), descs[::-1].copy())], None)
        elif which == "thresholds":
            rng = np.random.default_rng(7)
            d = rng.integers(0, 256, 32, dtype=np.uint8)
            pts = np.concatenate([FU.point_at_pixel(100.0 + 100.0 * k, 200.0) for k in range(4)])
            fr = RL.frame_of([100.0 + 100.0 * k for k in range(4)], [200.0] * 4, [FU.flip_bits(rng, d, n) for n in (63, 64, 65, 66)])
            return reloc_arrays(fr, [RL.cand_of(pts, np.stack([d] * 4))], None, th=3.0, orb_dist=64)
        else:
            cd, fr, kw = RL.contention_cases()[which][:3]
            return reloc_arrays(fr, [cd], None, check_ori=kw.get("check_ori", True))
        return reloc_arrays(fr, [cd], None)
    return make


def _bow_hand_tables():
    """The hand-worked tables of tests/test_bow_search_cpu.py and tests/test_bow_kf_search_cpu.py side by side, each in a node of its
    own (a node is a search of its own): a tie in the best distance; 20, 20, then 5; a single candidate at 49, 50 and 51; the ratio
    products 0.75 * 40, 0.75 * 41, 0.6f * 25 and 0.7f * 50; a row claimed earlier in its node; invalid rows; nodes on one side only;
    and, in angles, half-steps of the rotation bin.  -> side 1 (the keyframe / pKF1), side 2 (the frame / pKF2)"""
    D, Z = BW.desc_with_bits, BW.Z
    one, two, node = [], [], [0]

    def group(rows1, rows2):
        one.extend(r[:2] + (node[0],) + r[2:] for r in rows1)
        two.extend(r[:2] + (node[0],) + r[2:] for r in rows2)
        node[0] += 2                                                # (odd nodes stay empty on both sides: lower_bound steps)

    group([(Z, 0)], [(D(10), 0), (D(10, offset=100), 0)])
    group([(Z, 0)], [(D(20), 0), (D(20, offset=40), 0), (D(5, offset=200), 0)])
    for n in (49, 50, 51):
        group([(Z, 0)], [(D(n), 0)])
    for d1, d2 in ((30, 40), (30, 41), (15, 25), (35, 50), (3, 5)):   # (0.6f * 5 is a tie between 3.0f and the float above: 3.0f)
        group([(Z, 0)], [(D(d1), 0), (D(d2, offset=100), 0)])
    group([(Z, 0), (D(1), 0)], [(D(2), 0), (D(20, offset=64), 0), (D(60, offset=128), 0)])
    group([(Z, 0, 0), (Z, 0)], [(D(2), 0), (D(12, offset=64), 0, 0)])
    group([(Z, 0)], [])
    group([], [(Z, 0)])
    for ang in (45.0, 15.0, 75.0, 345.0, 359.99, 14.999, 15.001):
        group([(D(3, offset=(len(one) * 17) % 250), ang)], [(D(3, offset=(len(one) * 17) % 250), 0.0)])
    one.append((Z, 0, -1)); two.append((Z, 0, -1))
    return BK.table(one), BK.table(two)


def _bow_filter_tables():
    """tests/test_bow_kf_search_cpu.py: test_the_rotation_filter_does_not_give_a_taken_feature_back, as tables: row 0 of side 1 takes
    row 0 of side 2 and is then cleared by the rotation filter; row 1 (same node) still had to take its second choice."""
    D, Z = BW.desc_with_bits, BW.Z
    kf1 = [(Z, 90.0, 4), (D(1), 0.0, 4)]
    kf2 = [(D(2), 0.0, 4), (D(20, offset=64), 0.0, 4)]
    for i in range(20):
        d = D(3, offset=(i * 11) % 250)
        kf1.append((d, 0.0, 50 + i)); kf2.append((d, 0.0, 50 + i))
    return BK.table(kf1), BK.table(kf2)


def _bow_case(kind, kf_form, nnratio=0.75, ori=True):
    def make():
        if kind == "hand":
            one, two = _bow_hand_tables()
        elif kind == "filter":
            one, two = _bow_filter_tables()
        elif kind == "boundary":
            one, two = BK.boundary_case()
        else:
            rng = np.random.default_rng(kind)
            if kf_form:
                one, kfs = BK.batch_of(rng, 3, n1=250, nnodes=25, max_n2=300)
                return bow_kf_arrays(one, kfs + [BK.kf_pair_case(rng, 10, 200, 25)[1]], nnratio, ori)
            kd, ka, kn, kv, fd, fa, fn = BW.random_case(rng, 250, 250, 20)
            kfs = [(kd, ka, kn, kv)] + [BW.keyframe_of(rng, (fd, fa, fn), 200) for _ in range(3)]
            return bow_arrays(kfs, (fd, fa, fn), nnratio, ori)
        return bow_kf_arrays(one, [two], nnratio, ori) if kf_form else bow_arrays([one], two[:3], nnratio, ori)
    return make


def _init_case(which):
    def make():
        if which == "scene":
            t1, frames = IN.scene(np.random.default_rng(IN.SCENE_SEED), later=1)
            return init_arrays(t1, frames)
        if which == "chain":
            t1, frames = IN.chain_scene()
            return init_arrays(t1, frames)
        if which == "scene_small_window":
            t1, frames = IN.scene(np.random.default_rng(IN.SCENE_SEED + 1), nfam=120, later=1)
            return init_arrays(t1, frames, window=20, nnratio=0.75)
        if which == "tie_ratio_15":                                # with a ratio above 1 a tie in the best distance is accepted: the first
            t1 = IN.table([100], [100], [IN.ZERO])
            t2 = IN.table([103, 101], [100, 100], [IN.bits((0, 9)), IN.bits((100, 9))])
            return init_arrays(t1, [t2], window=10, nnratio=1.5)
        if which == "ratio_06":                                    # (float)5 * 0.6f rounds to 3.0f: 3 < 3.0f fails; in double it is 3.0000001
            t1 = IN.table([100, 300], [100, 100], [IN.ZERO, IN.ZERO])
            t2 = IN.table([101, 103, 301, 303], [100] * 4, [IN.bits((0, 3)), IN.bits((100, 5)), IN.bits((0, 3)), IN.bits((100, 6))])
            return init_arrays(t1, [t2], window=10, nnratio=0.6)
        t1, t2, prev, kw = IN.hand_cases()[which][:4]
        return init_arrays(t1, [t2], prev, window=kw["window"])
    return make


def _tri_seeded(seed, nkf, npts, nnodes):
    def make():
        poses = []
        t1, nbrs = TR.two_view_case(np.random.default_rng(seed), nkf, npts, nnodes=nnodes, poses=poses)
        return tri_arrays(t1, [n[0] for n in nbrs], poses)
    return make


def _tri_hand():
    """Rows in nodes of their own.  Neighbour 0 stands where the keyframe stands (identity rotations, equal translations): t12 is
    exactly 0, F12 is all zeros and den == 0 for every pair - nothing matches unless bCoarse.  Neighbour 1 has moved along x (the
    epipolar line of (x1, y1) is y2 = y1): equal distances on the line (the later one wins), a distance of exactly TH_LOW and
    TH_LOW + 1, a closer descriptor off the line, a feature of the neighbour matched by two of the keyframe."""
    D, Z = BW.desc_with_bits, BW.Z
    rows1, rows2 = [], []
    for k, (dists, dy) in enumerate((((10, 10), (0, 0)), ((50,), (0,)), ((51,), (0,)), ((0, 20), (40, 0)), ((5,), (0,)))):
        y = 60.0 + 60.0 * k
        rows1.append((200.0, y, 0, 0.0, Z, k))
        for j, (d, off) in enumerate(zip(dists, dy)):
            rows2.append((150.0 + 10 * j, y + off, 0, 0.0, D(d, offset=60 * j), k))
    rows1.append((300.0, 300.0, 0, 0.0, D(1), 4))                     # a second keyframe row in node 4: the same neighbour feature
    rows2[-1] = (150.0, 300.0, 0, 0.0, D(5), 4)
    rows1[4] = (200.0, 300.0, 0, 0.0, Z, 4)
    t1, t2 = TR.make_table(rows1), TR.make_table(rows2)
    I, t = np.eye(3), np.array([0.1, 0.0, 0.0])
    return tri_arrays(t1, [t2, t2], [(I, t, I, t), (I, np.zeros(3), I, np.array([0.5, 0.0, 0.0]))])


def _local_scene(ncur, nq=300, th=3.0, far=True):
    """The current frame of tests/helpers_matchers.py: dense_window_tables (ncur rows, seeded by ncur) and its query positions as the
    projections Frame::isInFrustum left in the map points, with levels, viewing cosines and depths of their own."""
    def make():
        q, qd, kp, desc, ur, occ, bounds, rng = HM.dense_window_tables(ncur, nq)
        track = np.zeros((nq, 8), f32)
        track[:, 0] = q["valid"]
        track[:, 1], track[:, 2], track[:, 3] = q["u"], q["v"], q["ur"]
        track[:, 4] = rng.uniform(1, 80, nq)
        track[:, 5] = rng.integers(0, FU.NLEVELS, nq)
        track[:, 6] = np.where(rng.random(nq) < 0.5, rng.uniform(0.9981, 1.0, nq), rng.uniform(0.5, 0.998, nq))
        occ3 = np.where(occ != 0, np.where(rng.random(len(occ)) < 0.7, 1, 2), 0)
        return local_arrays(kp, desc, ur, occ3, track, qd, rng.random(nq) < 0.05, bounds, th=th, far=far)
    return make


def _local_hand(nnratio=0.8):
    """tests/helpers_matchers.py: build_projection_cases' "local_map_ratio" and edge items in the form the reference call can take
    (th 4 and a viewing cosine of 1: radius 2.5 * 4 * 1 at level 0, window [-1, 0]): best / second best on one level or two at the
    float boundary of nnratio, 100 and 101 bits, the right-coordinate gate at |error| == radius, an occupied nearest keypoint, a row
    on mnMaxX's side of the image."""
    P = HM._Proj(34)
    for d1, d2, same in ((8, 10, True), (9, 10, True), (7, 10, True), (16, 20, True), (17, 20, True), (80, 100, True), (81, 100, True),
                         (40, 50, True), (41, 50, True), (9, 10, False), (50, 50, True), (50, 50, False), (100, 120, True), (7, 10, True),
                         (14, 20, True), (6, 10, True)):           # (0.7f * 10 rounds UP to 7.0f: 7 > 7.0f fails, in double it is 6.9999999)
        u, v = P.place(); i = P.query(u, v)
        P.key(u + 1, v, i, d2, octave=0); P.key(u, v, i, d1, octave=0 if same else 1)
    for bits in (99, 100, 101, 102, 101, 103, 110):
        P.item(bits)
    P.item(3, octave=1); P.item(3, ur=-1.0)
    u, v = P.place(); i = P.query(u, v, ur=u - 5.0); P.key(u, v, i, 3, ur=u - 15.0)
    u, v = P.place(); i = P.query(u, v, ur=u - 5.0); P.key(u, v, i, 3, ur=u - 15.5)
    u, v = P.place(); i = P.query(u, v); P.key(u, v, i, 2, occ=1); P.key(u + 2, v, i, 7)
    u, v = P.place(); i = P.query(u, v); P.key(u, v, i, 2, occ=1)
    u, v = P.place(); i = P.query(u, v); P.key(u, v, i, 2); j = P.query(u + 1, v); P.qd[j] = HM._flip(P.qd[i], 1); P.key(u + 3, v, i, 30)
    u, v = P.place(); i = P.query(u, v); P.key(u + 6, v, i, 5); P.key(u - 6, v, i, 5); P.key(u - 6, v - 6, i, 5)
    # equal distances on two levels (level 1: radius 12, octaves 0 and 1): the first in walking order is the best, the other the
    # second best on another level, so the match stands and says which came first
    u, v = P.place(); i = P.query(u, v, hi=1); P.key(u + 7, v, i, 5, octave=0); P.key(u - 7, v, i, 5, octave=1)
    i = P.query(640.0, 100.0); P.key(632.0, 100.0, i, 4)
    P.item(2, valid=0)
    t = P.tables()
    q = t["q"]
    track = np.zeros((len(q), 8), f32)
    track[:, 5] = np.maximum(q["max_level"], 0)
    track[:, 0], track[:, 1], track[:, 2], track[:, 3], track[:, 4], track[:, 6] = q["valid"], q["u"], q["v"], q["ur"], 10.0, 1.0
    return local_arrays(t["kp"], t["desc"], t["ur"], t["occ"], track, t["qd"], np.zeros(len(q), bool), t["bounds"], th=4.0, far=False, nnratio=nnratio)


def _frame_scene(ncur, motion, mono=False, nq=300):
    """A current frame of tests/helpers_matchers.py: dense_window_tables, and a last frame whose points project near its queries;
    motion: the last frame's camera centre in the current camera's frame (z beyond mb: forward, beyond -mb: backward)."""
    def make():
        q, qd, kp, desc, ur, occ, bounds, rng = HM.dense_window_tables(ncur, nq)
        cam = cam10(FU.CAM, mb=float(FU.CAM.bf) / float(FU.CAM.fx))
        cam[5:9] = bounds
        cur = FU.make_pose(FU.rot_xyz(*rng.uniform(-0.03, 0.03, 3)), rng.uniform(-0.3, 0.3, 3))
        R, t = cur[:9].reshape(3, 3).astype(f64), cur[9:12].astype(f64)
        z = rng.uniform(2.0, 20.0, nq) * np.where(rng.random(nq) < 0.05, -1.0, 1.0)
        pc = np.stack([(q["u"] - float(cam[2])) * z / float(cam[0]), (q["v"] - float(cam[3])) * z / float(cam[1]), z], 1)
        pos = (pc - t) @ R                                            # R^T (pc - t)
        Rl = FU.rot_xyz(*rng.uniform(-0.01, 0.01, 3)) @ R
        last = FU.make_pose(Rl, (Rl @ R.T) @ (t - np.asarray(motion, f64)))
        occ3 = np.where(occ != 0, np.where(rng.random(len(occ)) < 0.7, 1, 2), 0)
        return frame_arrays(kp, desc, ur, occ3, pos.astype(f32), qd, (rng.random(nq) > 0.1).astype(np.int32) * 2, rng.integers(0, FU.NLEVELS, nq),
                            q["angle"], rng.random(nq) < 0.9, rng.random(nq) < 0.05, cur, last, cam, th=7.0, mono=mono)
    return make


def _frame_hand():
    """tests/helpers_matchers.py: build_projection_cases' edge and rotation items in the form the reference call can take: identity
    poses and a camera with fx = fy = 1, cx = cy = 0, bf = 5, so that a point (u, v, 1) projects to (u, v) and ur = u - 5 exactly;
    th 10 at octave 0: radius 10, octaves [-1, 1].  100 and 101 bits, octaves 1 and 2, the right-coordinate gate at |error| ==
    radius, occupied rows, a point without observations, equal distances in three cells, projections on all four bounds, and the
    rotation groups of "proj_rot_two" (30 : 3 : 2 at 90, 180 and 270 degrees beside the items at 0), and a pair whose first query votes
    alone for bin 7: the filter clears its row after that row has sent the second query to its second choice."""
    P = HM._Proj(31)
    for bits in (99, 100, 101, 102):
        P.item(bits)
    P.item(3, octave=1); P.item(3, octave=2); P.item(3, ur=-1.0)
    u, v = P.place(); i = P.query(u, v, ur=u - 5.0); P.key(u, v, i, 3, ur=u - 15.0)
    u, v = P.place(); i = P.query(u, v, ur=u - 5.0); P.key(u, v, i, 3, ur=u - 15.5)
    u, v = P.place(); i = P.query(u, v); P.key(u, v, i, 2, occ=1); P.key(u + 2, v, i, 7)
    u, v = P.place(); i = P.query(u, v); P.key(u, v, i, 2, occ=1)
    u, v = P.place(); i = P.query(u, v, valid=3); P.key(u, v, i, 2); j = P.query(u + 1, v); P.qd[j] = HM._flip(P.qd[i], 1)
    u, v = P.place(); i = P.query(u, v); P.key(u, v, i, 2); j = P.query(u + 1, v); P.qd[j] = HM._flip(P.qd[i], 1); P.key(u + 3, v, i, 30)
    u, v = P.place(); i = P.query(u, v); P.key(u + 6, v, i, 5); P.key(u - 6, v, i, 5); P.key(u - 6, v - 6, i, 5)
    for uu, vv, kx, ky in ((640.0, 100.0, 632.0, 100.0), (0.0, 140.0, 3.0, 140.0), (100.0, 480.0, 100.0, 474.0), (140.0, 0.0, 140.0, 2.0)):
        i = P.query(uu, vv); P.key(kx, ky, i, 4)
    P.query(641.0, 100.0); P.query(100.0, -2.0)
    for bits in (101, 103, 110, 140):
        P.item(bits)
    for rot, n in ((90.0, 30), (180.0, 3), (270.0, 2), (0.0, 1)):
        for _ in range(n):
            P.item(1, angle=rot)
    # a row taken by a query of a filtered bin (rot 200, alone in bin 7) blocks the next query, which falls to its second choice
    u, v = P.place(); i = P.query(u, v, angle=200.0); P.key(u, v, i, 2, angle=0.0)
    j = P.query(u + 1, v, angle=90.0); P.qd[j] = HM._flip(P.qd[i], 1); P.key(u + 3, v, j, 30, angle=0.0)
    t = P.tables()
    q = t["q"]
    nq = len(q)
    pos = np.stack([q["u"], q["v"], np.ones(nq, f32)], 1)
    return frame_arrays(t["kp"], t["desc"], t["ur"], t["occ"], pos, t["qd"], np.where(q["valid"] == 3, 0, 2), np.zeros(nq, np.int32), q["angle"],
                        q["valid"] != 0, np.zeros(nq, bool), FU.IDENTITY, FU.IDENTITY, IDENTITY_CAM, th=10.0, mono=True)


def _frame_forms(ncur=400, most=24):
    """The points of frame_scene400 whose u differs in its bits between Pinhole::project (fx*x/z + cx, what this overload calls) and
    the inverse-depth form of the overload with match12 (fx*x*invz + cx), each with ONE keypoint at the edge of its window: a float x
    with |x - u| < radius under one form and not under the other (tests/test_sim3_projection_cpu.py: boundary_case's method)."""
    a = _frame_scene(ncur, (0.05, 0.0, 0.02))()
    case = FrameCase("", a, [])
    (q0, qd), (q1, _) = case.queries(a), case.queries(a, True)
    rows, keep = [], []
    for i in np.nonzero((q0["valid"] != 0) & (q0["u"] != q1["u"]) & (q0["u"] > 60) & (q0["u"] < 580) & (q0["v"] > 0) & (q0["v"] < 480))[0]:
        r, found = q0["radius"][i], None
        for sign in (1.0, -1.0):
            x = f32(q0["u"][i] + f32(sign) * r)
            for _ in range(8):
                x = np.nextafter(x, f32(-np.inf))
            for _ in range(16):
                if (abs(f32(x - q0["u"][i])) < r) != (abs(f32(x - q1["u"][i])) < r):
                    found = x
                    break
                x = np.nextafter(x, f32(np.inf))
            if found is not None:
                break
        if found is not None and all(abs(float(found) - k[0]) > 60 or abs(float(q0["v"][i]) - k[1]) > 60 for k in rows):
            rows.append((float(found), float(q0["v"][i]), int(a["last_octave"][i]), i))
            keep.append(i)
        if len(rows) == most:
            break
    assert len(rows) >= 5
    n = len(rows)
    a = dict(a)
    a.update({"cur_x": np.array([k[0] for k in rows], f32), "cur_y": np.array([k[1] for k in rows], f32),
              "cur_octave": np.array([k[2] for k in rows], np.int32), "cur_angle": a["last_angle"][keep].copy(), "cur_desc": a["mp_desc"][keep].copy(),
              "cur_uright": np.full(n, -1, f32), "cur_occ": np.zeros(n, np.uint8)})
    held = np.zeros(len(a["last_held"]), np.uint8)
    held[keep] = 1
    a["last_held"], a["last_outlier"] = held, np.zeros(len(held), np.uint8)
    return a


def _calls(prefix, n, suffixes=("",)):
    return ["%s%d%s" % (prefix, k, s) for k in range(n) for s in suffixes]


FORMS = ("_form0", "_form1")
CASES = [
    FuseCase("fuse_seed1", _fuse_seeded(1, 3, 250, 300), _calls("kf", 3) + _calls("sim3_kf", 3)),
    FuseCase("fuse_seed2", _fuse_seeded(2, 3, 200, 250), _calls("kf", 3) + _calls("sim3_kf", 3)),
    FuseCase("fuse_hand", _fuse_hand, _calls("kf", 3) + _calls("sim3_kf", 3), tags=("tie", "threshold", "max_x")),
    Sim3Case("sim3_seed1", _sim3_seeded(1, 3, 250, 300, 3.0, 1.0), _calls("kf", 3, FORMS)),
    Sim3Case("sim3_seed2", _sim3_seeded(2, 3, 200, 250, 5.0, 1.5), _calls("kf", 3, FORMS)),
    Sim3Case("sim3_thresholds", _sim3_hand("thresholds"), _calls("kf", 4, FORMS), tags=("threshold",)),
    Sim3Case("sim3_thresholds_ratio15", _sim3_hand("thresholds_ratio15"), _calls("kf", 4, FORMS), tags=("threshold",)),
    Sim3Case("sim3_edge", _sim3_hand("edge"), _calls("kf", 1, FORMS), tags=("max_x",)),
    Sim3Case("sim3_reversal", _sim3_hand("reversal"), _calls("kf", 2, FORMS)),
    Sim3Case("sim3_boundary", _sim3_hand("boundary"), _calls("kf", 1, FORMS)),
] + [Sim3Case("sim3_" + n, _sim3_hand(n), _calls("kf", 1, FORMS), tags=("tie",) if n == "listed_twice" else ())
     for n in ("second_best", "second_best_above_limit", "chain", "occupied", "skipped", "listed_twice")] + [
    RelocCase("reloc_seed1", _reloc_seeded(1, 3, 250, 300, 10.0, 100), _calls("c", 3)),
    RelocCase("reloc_seed2", _reloc_seeded(2, 3, 200, 250, 3.0, 64), _calls("c", 3)),
    RelocCase("reloc_thresholds", _reloc_hand("thresholds"), _calls("c", 1), tags=("threshold",)),
    RelocCase("reloc_edge", _reloc_hand("edge"), _calls("c", 1), tags=("max_x",)),
    RelocCase("reloc_tie", _reloc_hand("tie"), _calls("c", 1), tags=("tie",)),
    RelocCase("reloc_filtered_row", _reloc_hand("filtered_row"), _calls("c", 1), tags=("filtered_row",)),
    RelocCase("reloc_reversal", _reloc_hand("reversal"), _calls("c", 2)),
    RelocCase("reloc_behind", _reloc_hand("behind"), _calls("c", 1)),
] + [RelocCase("reloc_" + n, _reloc_hand(n), _calls("c", 1))
     for n in ("second_best", "second_best_above", "occupied", "invalid", "octave_plus_one", "octave_plus_two", "orientation_off")] + [
    BowCase("bow_seed5", _bow_case(5, False), _calls("kf", 4)),
    BowCase("bow_seed6_ratio09", _bow_case(6, False, 0.9), _calls("kf", 4)),
    BowCase("bow_hand", _bow_case("hand", False, 0.75, False), _calls("kf", 1), tags=("tie", "ratio", "threshold")),
    BowCase("bow_hand_ratio06", _bow_case("hand", False, 0.6), _calls("kf", 1), tags=("ratio",)),
    BowCase("bow_hand_ratio07", _bow_case("hand", False, 0.7), _calls("kf", 1), tags=("ratio",)),
    BowCase("bow_hand_ratio15", _bow_case("hand", False, 1.5), _calls("kf", 1), tags=("tie",)),
    BowCase("bow_filter", _bow_case("filter", False), _calls("kf", 1), tags=("filtered_row",)),
    BowKfCase("bowkf_seed5", _bow_case(5, True), _calls("kf", 4)),
    BowKfCase("bowkf_seed6_ratio09", _bow_case(6, True, 0.9), _calls("kf", 4)),
    BowKfCase("bowkf_hand", _bow_case("hand", True, 0.75, False), _calls("kf", 1), tags=("tie", "ratio", "threshold")),
    BowKfCase("bowkf_hand_ratio06", _bow_case("hand", True, 0.6), _calls("kf", 1), tags=("ratio",)),
    BowKfCase("bowkf_hand_ratio15", _bow_case("hand", True, 1.5), _calls("kf", 1), tags=("tie",)),
    BowKfCase("bowkf_boundary", _bow_case("boundary", True), _calls("kf", 1), tags=("threshold",)),
    BowKfCase("bowkf_filter", _bow_case("filter", True), _calls("kf", 1), tags=("filtered_row",)),
    InitCase("init_scene", _init_case("scene"), ["chain"]),
    InitCase("init_chain", _init_case("chain"), ["chain"]),
    InitCase("init_scene_small_window", _init_case("scene_small_window"), ["chain"]),
] + [InitCase("init_" + n, _init_case(n), ["chain"], tags={"equal_distance": ("tie",), "ratio_45_50_45_51": ("ratio",),
                                                           "th_low_50_51": ("threshold",), "histogram_counts_evicted": ("filtered_row",),
                                                           "ratio_06": ("ratio",), "tie_ratio_15": ("tie",)}.get(n, ()))
     for n in ("eviction", "equal_distance", "left_out_would_fail_ratio", "ratio_45_50_45_51", "th_low_50_51", "window_edge", "octave_1",
               "outside_the_grid", "prev_matched_elsewhere", "histogram_counts_evicted", "ratio_06", "tie_ratio_15")] + [
    TriCase("tri_seed11", _tri_seeded(11, 4, 120, 12), ["n%d_s%d%d%d" % ((k,) + s) for k in range(4) for s in TRI_SETTINGS]),
    TriCase("tri_seed12", _tri_seeded(12, 2, 150, 2), ["n%d_s%d%d%d" % ((k,) + s) for k in range(2) for s in TRI_SETTINGS]),
    TriCase("tri_hand", _tri_hand, ["n%d_s%d%d%d" % ((k,) + s) for k in range(2) for s in TRI_SETTINGS], tags=("tie", "threshold")),
    LocalCase("local_scene400", _local_scene(400), ["call"]),
    LocalCase("local_scene300_th1", _local_scene(300, nq=250, th=1.0, far=False), ["call"]),
    LocalCase("local_hand", _local_hand, ["call"], tags=("tie", "ratio", "threshold")),
    LocalCase("local_hand_ratio07", lambda: _local_hand(0.7), ["call"], tags=("ratio",)),
    FrameCase("frame_scene400", _frame_scene(400, (0.05, 0.0, 0.02)), ["call"]),
    FrameCase("frame_scene350_forward", _frame_scene(350, (0.0, 0.0, 0.5), nq=250), ["call"]),
    FrameCase("frame_scene300_backward", _frame_scene(300, (0.0, 0.0, -0.5), nq=250), ["call"]),
    FrameCase("frame_scene250_mono", _frame_scene(250, (0.0, 0.0, 0.5), mono=True, nq=200), ["call"]),
    FrameCase("frame_hand", _frame_hand, ["call"], tags=("tie", "threshold", "filtered_row", "max_x")),
    FrameCase("frame_forms", lambda: _frame_forms(), ["call"]),
]
BY_NAME = {c.name: c for c in CASES}
FUNCTIONS = ("fuse", "sim3", "reloc", "bow", "bow_kf", "init", "tri", "local", "frame")


def same(want, got):
    """Exact equality of two results of expected() / restate() / device(): nested tuples and lists of arrays and integers."""
    if isinstance(want, (tuple, list)):
        return isinstance(got, (tuple, list)) and len(want) == len(got) and all(same(w, g) for w, g in zip(want, got))
    w, g = np.asarray(want), np.asarray(got)
    return w.shape == g.shape and (w.tobytes() == g.astype(w.dtype).tobytes() if w.dtype.kind == "f" else np.array_equal(w, g))


def exit_counts(cases=None):
    """{function: Counter}: how often every exit of the restatements' EXITS was taken over the fixture corpus (the scalar
    restatement counts them; test_ref_pin_match.py holds it to the fixtures)."""
    counts = {}
    for c in CASES if cases is None else cases:
        a, _ = load_fixture(c.name)
        ex = counts.setdefault(c.fn, Counter())
        for call in c.calls:
            c.restate(a, call, exits=ex)
    return counts
