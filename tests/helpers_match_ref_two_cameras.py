"""The two-camera pin's corpus and fixtures: the reference's own src/CameraModels/KannalaBrandt8.cpp, compiled where it lies into
oracle/_ref/pli_ref_match (oracle/Makefile: ref_match, match_KannalaBrandt8.o; the stand-in it compiles against is
oracle/ref_recipe/match_shim), run over tables of points, pixels and keypoint pairs (the driver's function "kb8").

  KB8_CASES             the named cases, one per rig of helpers_geometry.RIGS: points and pixels for project / unproject of both
                        cameras, and the pairs of helpers_geometry.fisheye_cases (every exit of TriangulateMatches, each gate decided
                        with the margins of helpers_geometry) for cam1.TriangulateMatches(&cam2, ...)
  TRI2_CASES            SearchForTriangulation with mpCamera2 on both keyframes (the driver's "tri2"): a hand case and the corpus of
                        test_triangulation_two_cameras_cpu.py, every neighbour under bOnlyStereo / bCoarse / mbCheckOrientation all ways
  BOW2_CASES            SearchByBoW(pKF, F, ...) with F.Nleft != -1 ("bow2"): the known answers of test_bow_two_cameras_cpu.py as one
                        hand table, without and with the rotation filter, and its seeded corpus under its three settings
  FUSE2_CASES           Fuse(pKF, vpMapPoints, th, bRight) for a two-camera keyframe ("fuse2"): seven hand cases, one named edge each, and
                        two scenes of test_fuse_two_cameras_cpu.fuse2_case with Nright <= Nleft
  LOCAL2_CASES          SearchByProjection(F, vpMapPoints, ...) with F.Nleft != -1 ("local2"): two hand cases and three seeded scenes; the
                        function had no Python restatement, Local2Case.restate is one, with its misreading switches
  FRAME2_CASES          SearchByProjection(CurrentFrame, LastFrame, ...) with CurrentFrame.Nleft != -1 ("frame2"): projections that are
                        exact in float, four hand cases (neutral, forward, backward, no orientation check) and four seeded scenes
  save_fixture / load_fixture   tests/golden/match_ref_two_cameras/<case>.npz: "in/<array>" and "out/call/<array>"
  generate              records the fixtures by running the program (not a test; `python tests/helpers_match_ref_two_cameras.py`)
  project32 / unproject32        KannalaBrandt8::project / unproject in float32 with the libm results handed in, so that a test can ask
                        which 1-ulp change of atan2f / tanf explains a recorded value

Nothing here reads the reference tree; generate and run_reference need the program oracle/Makefile built from it.  The fixtures
record what that program computed with the C library it was linked to (glibc 2.35: its atan2f and tanf are not correctly rounded).
"""
import io
import math
import os
import subprocess
import tempfile
import zipfile
from collections import Counter

import numpy as np

import helpers_geometry as G
import helpers_matchers as HM
import test_bow_two_cameras_cpu as B2
import test_fuse_two_cameras_cpu as F2
import test_triangulation_two_cameras_cpu as T2
import test_two_camera_projection_cpu as P2
from helpers_match_ref import mat44, rows_after, REF_EXE, ROOT, _bow_objects, fuse_apply, points_bag, points_of, rows_from_ops, FU, _fn, _params, concat_points, extra_points, keypoints, read_bag, same, table_bag, write_bag  # noqa: F401

GOLD_DIR = os.path.join(ROOT, "tests", "golden", "match_ref_two_cameras")
f32, f64 = np.float32, np.float64
SIZE_CAP = (1 << 20) + (1 << 16)
LIBM_HINT = ("the kb8 fixtures record glibc 2.35's atan2f / tanf, which are not correctly rounded: a program linked to another C library "
             "may differ in the last bit at the residue inputs (DESIGN.md §2); record the fixtures again there with generate()")
MAX_ROWS, MAX_POINTS, MAX_TABLES = 400, 400, 4


FUNCTIONS = ("kb8", "tri2", "bow2", "fuse2", "local2", "frame2")
_REF_FUNCTIONS = None


def ref_functions():
    """What `pli_ref_match --functions` lists (asked once): empty where the program is absent or was built from a recipe that
    predates the two-camera functions (such a program only knows `CASE RESULT` and answers with its usage)."""
    global _REF_FUNCTIONS
    if _REF_FUNCTIONS is None:
        _REF_FUNCTIONS = frozenset()
        if os.path.exists(REF_EXE):
            try:
                r = subprocess.run([REF_EXE, "--functions"], capture_output=True, text=True, timeout=60)
                if r.returncode == 0:
                    _REF_FUNCTIONS = frozenset(r.stdout.split())
            except (OSError, subprocess.SubprocessError):
                pass
    return _REF_FUNCTIONS


def run_reference(bag, exe=REF_EXE):
    """One call of the reference program: the result arrays by name.  A call that fails says what the program wrote."""
    with tempfile.TemporaryDirectory() as d:
        req, rsp = os.path.join(d, "case"), os.path.join(d, "result")
        write_bag(req, bag)
        r = subprocess.run([exe, req, rsp], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, "pli_ref_match exit %d: %s" % (r.returncode, r.stderr.strip()[-300:])
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


# ------------------------------------------------------------------------------------------------------------------- kb8 cases
def _points(rng, n):
    """Camera-frame points over the whole sphere of directions (z < 0 included), 0.2 - 20 m, then the named edges."""
    th, ph, rho = rng.uniform(0.0, 3.1, n), rng.uniform(0, 2 * np.pi, n), np.exp(rng.uniform(np.log(0.2), np.log(20.0), n))
    P = np.stack([rho * np.sin(th) * np.cos(ph), rho * np.sin(th) * np.sin(ph), rho * np.cos(th)], 1)
    edges = [(0, 0, 1), (0, 0, 2.5), (0, 0, -1), (0, 0, 0), (0, 1, 1), (0, -1, 1), (0, 2, -1), (1, 0, 1), (-1, 0, 1), (-2, 0, -1),
             (1, 1, 0), (-1, 1, 0), (0, 1, 0), (-1, 0, 0), (1e-6, 0, 1), (0, -1e-6, 1), (1e-4, 1e-4, 1), (3, -4, -0.5), (-0.0, 1, 1),
             (1, -0.0, 1), (-1, -0.0, 1), (-1, 0.0, -1), (-1, -0.0, -1)]
    return np.concatenate([P, np.array(edges, np.float64)]).astype(f32)


def _pixels(rng, cam, n):
    """Pixels over the image and beyond it (theta_d up to the clamp at pi / 2 and past it), a dense disc round the principal point
    (Newton stops after one step), the principal point itself (theta_d <= 1e-8) and its neighbours one float away."""
    fx, fy, cx, cy = [f32(c) for c in cam[:4]]
    r, ph = rng.uniform(0.0, 1.7, n) * float(fx), rng.uniform(0, 2 * np.pi, n)
    wide = np.stack([cx + r * np.cos(ph), cy + r * np.sin(ph)], 1)
    r, ph = rng.uniform(0.0, 0.08, n // 4) * float(fx), rng.uniform(0, 2 * np.pi, n // 4)
    near = np.stack([cx + r * np.cos(ph), cy + r * np.sin(ph)], 1)
    edges = [(cx, cy), (np.nextafter(cx, f32(1e9)), cy), (cx, np.nextafter(cy, f32(-1e9))), (cx, 0), (0, cy), (0, 0), (511, 511),
             (cx + f32(400), cy), (cx, cy - f32(900)), (cx + f32(1e-6) * fx, cy)]
    return np.concatenate([wide, near, np.array(edges, np.float64)]).astype(f32)


# per rig: the pairs of helpers_geometry.fisheye_cases (seed and counts), and the tolerance class of helpers_geometry
_KB8 = {
    "tumvi": dict(seed=131, n_ok=50, n_far=50, n_rev=14, n_noise=80, n_centre=4),
    "tumvi_corner": dict(rig="tumvi", seed=137, n_corner=24, n_ok=6, tol="corner"),
    "pinhole": dict(seed=133, n_ok=40, n_far=40, n_rev=8, n_noise=60),
    "micro": dict(seed=167, n_ok=50, depth_scale=1e-4),
    "wide": dict(seed=134, n_z2=20, n_ok=10),
    "fold": dict(seed=136, n_z2=12, z2_on_axis=True),
}


class Kb8Case:
    fn = "kb8"
    calls = ("call",)

    def __init__(self, name):
        self.name = "kb8_" + name
        spec = dict(_KB8[name])
        self.rig = spec.pop("rig", name)
        self.tol = spec.pop("tol", "default")
        self.spec = spec

    def arrays(self):
        """The case's inputs.  No pair may be undecided (a gate inside helpers_geometry's margins): the seeds are chosen so that the
        draw holds none, and nothing is left out."""
        cam1, cam2, R12, t12 = G.RIGS[self.rig]
        rng = np.random.default_rng(self.spec["seed"] + 1000)
        sigma2 = G.fisheye_sigma2()
        pairs = G.fisheye_cases(self.rig, **self.spec)
        for c in pairs:
            lab, mg, _ = G.fisheye_expect(c["kp1"], c["kp2"], cam1, cam2, R12, t12, sigma2)
            assert not G.fisheye_undecided(lab, mg, self.tol), (self.name, lab, mg)
        assert 2 <= len(pairs) <= MAX_ROWS // 2
        o1 = np.array([c["kp1"][2] for c in pairs], np.int32)
        o2 = np.array([c["kp2"][2] for c in pairs], np.int32)
        return {
            "cam1": np.asarray(cam1, f32), "cam2": np.asarray(cam2, f32), "R12": np.asarray(R12, f32).reshape(9),
            "t12": np.asarray(t12, f32).reshape(3), "points": _points(rng, 200), "pixels": _pixels(rng, cam1, 240),
            "kp1": np.array([c["kp1"][:2] for c in pairs], f32), "kp2": np.array([c["kp2"][:2] for c in pairs], f32),
            "o1": o1, "o2": o2, "sigma": sigma2[o1].astype(f32), "unc": sigma2[o2].astype(f32),
        }

    def bag(self, a, call="call"):
        b = {k: a[k] for k in ("cam1", "cam2", "R12", "t12", "points", "pixels", "kp1", "kp2", "sigma", "unc")}
        b["fn"] = np.frombuffer(b"kb8", np.uint8)
        b["params"] = np.array([0.6, 1.0], np.float64)
        return b

    def labels(self, a):
        """The float64 model's exit and margins per pair (helpers_geometry.fisheye_expect)."""
        sigma2 = G.fisheye_sigma2()
        return [G.fisheye_expect((a["kp1"][i, 0], a["kp1"][i, 1], a["o1"][i]), (a["kp2"][i, 0], a["kp2"][i, 1], a["o2"][i]), a["cam1"],
                                 a["cam2"], a["R12"], a["t12"], sigma2) for i in range(len(a["kp1"]))]

    def tables(self, a):
        """The pairs as two keypoint tables for ComputeStereoFishEyeMatches: no mono rows, left row i and right row i share code row
        i (Hamming distance >= 128 from every other row), so the matching stage pairs row i with row i."""
        n = len(a["kp1"])
        kpL, kpR = np.zeros(n, G.KEYPOINT_DT), np.zeros(n, G.KEYPOINT_DT)
        kpL["x"], kpL["y"], kpL["octave"] = a["kp1"][:, 0], a["kp1"][:, 1], a["o1"]
        kpR["x"], kpR["y"], kpR["octave"] = a["kp2"][:, 0], a["kp2"][:, 1], a["o2"]
        d = G.code_rows(n)
        return kpL, d, kpR, d.copy()


KB8_CASES = [Kb8Case(n) for n in _KB8]


# ------------------------------------------------------------------ SearchForTriangulation with mpCamera2 on both keyframes
TRI2_FIELDS = T2.Table._fields
TRI2_SETTINGS = [(os_, co, ori) for os_ in (0, 1) for co in (0, 1) for ori in (0, 1)]


def _pose15(p):
    """Rcw row major, tcw, Ow = -Rcw.t() * tcw (one gemm, alpha -1), what the driver's table takes as R, t, Ow."""
    return np.concatenate([p.R.reshape(9), p.t.reshape(3), p.centre().reshape(3)]).astype(f32)


def tri2_arrays(t1, nbrs, pose1, poses2, settings=TRI2_SETTINGS):
    a = {"settings": np.array(settings, np.int32).reshape(-1, 3), "kb1": np.asarray(T2.CAMS[0], f32), "kb2": np.asarray(T2.CAMS[1], f32),
         "Tlr": np.hstack([T2.TLR_R, T2.TLR_T.reshape(3, 1)]).astype(f32), "pose1": _pose15(pose1)}
    a.update({"t1_" + f: np.asarray(v) for f, v in zip(TRI2_FIELDS, t1)})
    for k, (nb, p2) in enumerate(zip(nbrs, poses2)):
        a.update({"n%d_%s" % (k, f): np.asarray(v) for f, v in zip(TRI2_FIELDS, nb.t2)})
        a["n%d_pose2" % k], a["n%d_rel" % k], a["n%d_ep" % k] = _pose15(p2), np.asarray(nb.rel, f32), np.asarray(nb.ep, np.float64)
    a["t1_nleft"] = np.array([t1.nleft], np.int32)
    for k, nb in enumerate(nbrs):
        a["n%d_nleft" % k] = np.array([nb.t2.nleft], np.int32)
    return a


class Tri2Case:
    """SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo, bCoarse) with mpCamera2 on both keyframes, one call per
    neighbour and setting ("n<k>_s<onlyStereo><coarse><checkOrientation>").  The reference forms the four relative poses itself,
    from the keyframes' poses and mTlr; n<k>_rel is what test_triangulation_two_cameras_cpu.relative_poses makes of the same poses,
    for the restatements and the device."""
    fn = "tri2"
    exits = T2.EXITS

    def __init__(self, name, make, tags=()):
        self.name, self._make, self._a, self.tags, self._gates = name, make, None, tuple(tags), {}

    def arrays(self):
        if self._a is None:
            self._a = self._make()
        return self._a

    @property
    def calls(self):
        a = load_fixture(self.name)[0] if os.path.exists(fixture_path(self.name)) else self.arrays()
        nk = sum(1 for k in a if k.endswith("_pose2"))
        return ["n%d_s%d%d%d" % ((k,) + tuple(s)) for k in range(nk) for s in a["settings"]]

    def _call(self, call):
        k, s = call[1:].split("_s")
        return int(k), tuple(int(c) for c in s)

    def tables(self, a, k):
        tab = lambda pre: T2.Table(*[a[pre + f] if f != "nleft" else int(a[pre + f][0]) for f in TRI2_FIELDS])
        return tab("t1_"), T2.Neighbour(tab("n%d_" % k), a["n%d_rel" % k], a["n%d_ep" % k])

    def gate(self, a, k, rules=T2.REF):
        """The float64 gate of (pKF1, neighbour k), remembered: every setting of the pair asks the same pairs."""
        if (k, rules) not in self._gates:
            t1, nb = self.tables(a, k)
            self._gates[(k, rules)] = (t1, nb, T2.Gate(t1, nb, rules))
        return self._gates[(k, rules)]

    def bag(self, a, call):
        k, (os_, co, ori) = self._call(call)
        t1, nb = self.tables(a, k)
        bag = {"fn": _fn("tri2"), "params": _params(0.6, ori, os_, co)}
        base, bags = 0, []
        for pre, t, pose in zip(("t0_", "t1_"), (t1, nb.t2), (a["pose1"], a["n%d_pose2" % k])):
            n = len(t.node)
            mp = np.where(t.has_mp != 0, base + np.arange(n), -1).astype(np.int32)
            base += n
            bags.append(extra_points(n))
            bag.update(table_bag(pre, t.x, t.y, t.octave, t.angle, t.desc, np.zeros(10, f32), node=t.node, mp=mp, R=pose[:9].reshape(3, 3),
                                 t=pose[9:12], Ow=pose[12:15], nleft=np.array([t.nleft], np.int32), kb1=a["kb1"], kb2=a["kb2"], Tlr=a["Tlr"]))
            bag[pre + "sigma2"] = T2.SIGMA2.astype(f32)                    # mvLevelSigma2 as the restatements' gate reads it
        bag.update(concat_points(*bags))
        return bag

    def expected(self, a, call, res):
        """-> vMatches12[n1] (from vMatchedPairs, which lists them by idx1), nmatches"""
        m = np.full(len(a["t1_node"]), -1, np.int32)
        pairs = res["pairs"].reshape(-1, 2)
        assert (np.diff(pairs[:, 0]) > 0).all()
        m[pairs[:, 0]] = pairs[:, 1]
        return m, int(res["ret"][0])

    def restate(self, a, call, fast=False, exits=None, rules=T2.REF):
        k, (os_, co, ori) = self._call(call)
        t1, nb, gate = self.gate(a, k, rules)
        if fast:
            return T2.search_closed(t1, nb, bool(os_), bool(co), bool(ori), gate)
        return T2.search_scalar(t1, nb, bool(os_), bool(co), bool(ori), exits, gate)

    def undecided(self, a):
        """Pairs that reach the gate inside its decided margin, over all neighbours (must be 0)."""
        n = 0
        for k in range(sum(1 for key in a if key.endswith("_pose2"))):
            t1, nb, gate = self.gate(a, k)
            n += sum(bool(gate.look(i1, i2)[2]) for i1, i2, _ in T2.candidates(t1, nb.t2))
        return n

    def device(self, fe, a, calls):
        out = {}
        kf = lambda t: (keypoints(t.x, t.y, t.octave, t.angle), t.desc, t.node, t.has_mp, t.nleft)
        for s in sorted({self._call(c)[1] for c in calls}):
            mine = [c for c in calls if self._call(c)[1] == s]
            t1 = self.tables(a, 0)[0]
            nbs = [kf(nb.t2) + (nb.rel,) for nb in (self.tables(a, self._call(c)[0])[1] for c in mine)]
            m, n = fe.search_for_triangulation_two_cameras(kf(t1), nbs, a["kb1"], a["kb2"], bool(s[1]), bool(s[2]), bool(s[0]))
            for j, c in enumerate(mine):
                m1, n1 = fe.search_for_triangulation_two_cameras(kf(t1), nbs[j:j + 1], a["kb1"], a["kb2"], bool(s[1]), bool(s[2]), bool(s[0]))
                out[c] = ((m[j], int(n[j])), (m1[0], int(n1[0])))
        return out


def _tri2_corpus():
    t1, nbrs, redrawn = T2.corpus()
    assert redrawn == 0
    return tri2_arrays(t1, nbrs, T2.POSE_A, [T2.POSE_B, T2.POSE_C, T2.POSE_B])


def _tri2_hand():
    """One point in front of both rigs and its four images (test_triangulation_two_cameras_cpu._one_point), by hand:
      row 0 of pKF1 (left)   the point's left AND right image in pKF2 at distance 0 (rows 0 and 4): ll and lr both pass, the later
                             idx2 wins the tie -> 4
      row 1 (left)           the left image at distance exactly TH_LOW = 50 -> 1 (ll)
      row 2 (right)          the left image at distance 3 and the right one at 10 -> 3 (rl decides)
      row 3 (right)          a keypoint nowhere near (row 2, distance 0: TriangulateMatches <= 0.0001f alone turns it away) and the
                             right image at distance 20 -> 6 (rr); bCoarse skips the gate -> 2
    bOnlyStereo: nothing (bStereo1 is false with a second camera)."""
    rel, l1, r1, l2, r2 = T2._one_point()
    Z, bits = T2.Z, T2.desc_with_bits
    away = (f32(400.0), f32(90.0), 2, 0.0)
    t1 = T2.make_table([l1 + (Z, 4), l1 + (Z, 6), r1 + (Z, 5), r1 + (Z, 7)], 2)
    t2 = T2.make_table([l2 + (Z, 4), l2 + (bits(50), 6), away + (Z, 7), l2 + (bits(3), 5), r2 + (Z, 4), r2 + (bits(10), 5), r2 + (bits(20), 7)], 4)
    nb = T2.Neighbour(t2, rel, T2.epipole(T2.POSE_A, T2.POSE_B))
    for coarse, want in ((False, [4, 1, 3, 6]), (True, [4, 1, 3, 2])):
        m, n = T2.search_scalar(t1, nb, coarse=coarse)
        assert m.tolist() == want and n == 4, (coarse, m)
    return tri2_arrays(t1, [nb], T2.POSE_A, [T2.POSE_B])


TRI2_CASES = [Tri2Case("tri2_hand", _tri2_hand, tags=("tie", "threshold", "combos", "gate_alone", "coarse", "only_stereo")),
              Tri2Case("tri2_corpus", _tri2_corpus)]


# ------------------------------------------------------------------------------ SearchByBoW(pKF, F, ...) with F.Nleft != -1
def _two_camera_table(pre, desc, angle, node, nleft, mp=None):
    """A table of the driver without geometry (the search reads descriptors, angles and nodes): both cameras' rows, the left first."""
    n = len(node)
    z = np.zeros(n, f32)
    return table_bag(pre, z, z, np.zeros(n, np.int32), angle, desc, np.zeros(10, f32), node=np.asarray(node, np.int32), mp=mp,
                     nleft=np.array([nleft], np.int32), kb1=np.asarray(T2.CAMS[0], f32), kb2=np.asarray(T2.CAMS[1], f32),
                     Tlr=np.hstack([T2.TLR_R, T2.TLR_T.reshape(3, 1)]).astype(f32), R=np.eye(3, dtype=f32), t=np.zeros(3, f32), Ow=np.zeros(3, f32))


def bow2_arrays(kfs, frame, f_nleft, nnratio=0.7, check_ori=True):
    """kfs: [(desc, angle, node, valid)], frame: (desc, angle, node) as tests/test_bow_two_cameras_cpu.py has them."""
    a = {"th": _params(nnratio, check_ori), "f_desc": np.asarray(frame[0], np.uint8).reshape(-1, 32), "f_angle": np.asarray(frame[1], f32),
         "f_node": np.asarray(frame[2], np.int32), "f_nleft": np.array([f_nleft], np.int32)}
    for k, (d, ang, node, valid) in enumerate(kfs):
        a.update({"kf%d_desc" % k: np.asarray(d, np.uint8).reshape(-1, 32), "kf%d_angle" % k: np.asarray(ang, f32),
                  "kf%d_node" % k: np.asarray(node, np.int32), "kf%d_valid" % k: np.asarray(valid, np.uint8)})
    return a


class Bow2Case:
    """SearchByBoW(pKF, F, vpMapPointMatches) with F.Nleft != -1, one call per keyframe ("kf<k>").  The map point of keyframe row i
    is object i.  The keyframe is a two-camera table too (NLeft = half its rows): its keypoint is read from mvKeys or mvKeysRight
    (:379-382), which the restatements take as one table of angles."""
    fn = "bow2"
    exits = B2.EXITS

    def __init__(self, name, make, tags=()):
        self.name, self._make, self._a, self.tags = name, make, None, tuple(tags)

    def arrays(self):
        if self._a is None:
            self._a = self._make()
        return self._a

    @property
    def calls(self):
        a = load_fixture(self.name)[0] if os.path.exists(fixture_path(self.name)) else self.arrays()
        return ["kf%d" % k for k in range(sum(1 for key in a if key.endswith("_valid")))]

    def kf(self, a, k):
        return tuple(a["kf%d_%s" % (k, f)] for f in ("desc", "angle", "node", "valid"))

    def frame(self, a):
        return a["f_desc"], a["f_angle"], a["f_node"], int(a["f_nleft"][0])

    def bag(self, a, call):
        d, ang, node, valid = self.kf(a, int(call[2:]))
        mp, bad = _bow_objects(valid, 0)
        bag = {"fn": _fn("bow2"), "params": _params(a["th"][0], a["th"][1])}
        bag.update(points_bag(np.zeros(len(node), FU.FUSE_POINT_DT), np.zeros((len(node), 32), np.uint8), bad=bad))
        bag.update(_two_camera_table("t0_", d, ang, node, len(node) // 2, mp=mp))
        bag.update(_two_camera_table("t1_", a["f_desc"], a["f_angle"], a["f_node"], int(a["f_nleft"][0])))
        return bag

    def expected(self, a, call, res):
        """-> matches[nf] (the keyframe's row), nmatches"""
        return res["matches"].astype(np.int32), int(res["ret"][0])

    def restate(self, a, call, fast=False, exits=None, rules=B2.REF):
        if fast:
            return B2.search_closed(*self.kf(a, int(call[2:])), *self.frame(a), a["th"][0], bool(a["th"][1]))
        return B2.search_scalar(*self.kf(a, int(call[2:])), *self.frame(a), a["th"][0], bool(a["th"][1]), exits, rules)

    def device(self, fe, a, calls):
        kfs = [self.kf(a, int(c[2:])) for c in calls]
        fd, fa, fn, nl = self.frame(a)
        m, n = fe.search_by_bow_two_cameras(kfs, fd, fa, fn, nl, a["th"][0], bool(a["th"][1]))
        out = {}
        for j, c in enumerate(calls):
            m1, n1 = fe.search_by_bow_two_cameras(kfs[j:j + 1], fd, fa, fn, nl, a["th"][0], bool(a["th"][1]))
            out[c] = ((m[j], int(n[j])), (m1[0], int(n1[0])))
        return out


BOW2_HAND_NLEFT = 18
BOW2_HAND_WANT = [-1, -1, -1, 2, -1, -1] + list(range(4, 16)) + [-1, 1, 2, -1, 3] + list(range(4, 16))      # without the rotation filter


def _bow2_hand(nnratio=0.7, check_ori=False):
    """One keyframe, one frame, by hand (the known answers of test_bow_two_cameras_cpu.py in one table).  Keyframe rows 0-3 are zero
    descriptors in nodes 7, 3, 5, 9:
      node 7   left 51 bits away, right 0: no left candidate within TH_LOW, so the right best stays unmatched
      node 3   left 30 and 40 (30 < 0.7 * 40 fails), right 10: the right match is taken where the left failed its ratio test
      node 5   left 5; right 10 and 10: a ratio test would reject the right match, it is taken (the first listed), the left too
      node 9   left 8 and 8 (a tie: strict <, the first stays best, the ratio fails), right 2
    rows 4-15: twelve features with their left and right copies in nodes of their own, the last turned by 90 degrees: with the
    rotation filter its two matches, one per camera, are removed."""
    Z, bits = B2.Z, B2.desc_with_bits
    kf = [(Z, 0.0, 7), (Z, 0.0, 3), (Z, 0.0, 5), (Z, 0.0, 9)]
    left = [(bits(51), 0.0, 7), (bits(30), 0.0, 3), (bits(40, offset=60), 0.0, 3), (bits(5), 0.0, 5), (bits(8), 0.0, 9), (bits(8, offset=100), 0.0, 9)]
    right = [(Z, 0.0, 7), (bits(10, offset=120), 0.0, 3), (bits(10, offset=60), 0.0, 5), (bits(10, offset=120), 0.0, 5), (bits(2, offset=200), 0.0, 9)]
    for i in range(12):
        d = bits(3, offset=(i * 17) % 250)
        kf.append((d, 90.0 if i == 11 else 0.0, 100 + i))
        left.append((d, 0.0, 100 + i))
        right.append((d, 0.0, 100 + i))
    assert len(left) == BOW2_HAND_NLEFT
    col = lambda rows, i, dt: np.array([r[i] for r in rows], dt)
    kfs = [(col(kf, 0, np.uint8).reshape(-1, 32), col(kf, 1, f32), col(kf, 2, np.int32), np.ones(len(kf), np.uint8))]
    f = left + right
    frame = (col(f, 0, np.uint8).reshape(-1, 32), col(f, 1, f32), col(f, 2, np.int32))
    m, n = B2.search_scalar(*kfs[0], *frame, BOW2_HAND_NLEFT, 0.7, False)
    assert m.tolist() == BOW2_HAND_WANT, m.tolist()
    return bow2_arrays(kfs, frame, BOW2_HAND_NLEFT, nnratio, check_ori)


def _bow2_seeded(nnratio, check_ori):
    frame, kfs = B2.corpus(3)
    return bow2_arrays(kfs, frame, B2.F_NLEFT, nnratio, check_ori)


BOW2_CASES = [Bow2Case("bow2_hand", _bow2_hand, tags=("unmatched_right", "right_after_left_failed", "right_no_ratio", "tie")),
              Bow2Case("bow2_hand_filter", lambda: _bow2_hand(0.7, True), tags=("filtered",))] + \
             [Bow2Case("bow2_seeded_r%02d_o%d" % (int(r * 10), o), (lambda r=r, o=o: _bow2_seeded(r, o))) for r, o in B2.SETTINGS]


# ------------------------------------------------------------------------ Fuse(pKF, vpMapPoints, th, bRight) with NLeft != -1
def fuse2_arrays(pts, descs, kf, skip=None, th=3.0, bounds=F2.BOUNDS, sides=(0, 1)):
    """One keyframe of two cameras (F2.KF2) and the list's points.  Frame.cc:1589 leaves mvuRight with Nleft entries and Fuse reads
    mvuRight[idx] with the camera-local idx of either camera (:1533): every case here has Nright <= Nleft, so that the read stays
    inside the vector the reference would have."""
    nmp = len(pts)
    assert len(kf.x) - kf.nleft <= kf.nleft and len(kf.x) <= MAX_ROWS and nmp <= MAX_POINTS
    a = {"th": _params(th), "bounds": np.array(bounds, f32), "nmp": np.array([nmp], np.int32), "sides": np.array(sides, np.int32),
         "skip": np.zeros((2, nmp), np.uint8) if skip is None else np.asarray(skip, np.uint8).reshape(2, nmp),
         "kf_x": kf.x, "kf_y": kf.y, "kf_octave": kf.octave, "kf_desc": kf.desc, "kf_nleft": np.array([kf.nleft], np.int32), "kf_pose": kf.pose,
         "kb1": np.asarray(F2.CAMS[0], f32), "kb2": np.asarray(F2.CAMS[1], f32), "Tlr": np.hstack([T2.TLR_R, T2.TLR_T.reshape(3, 1)]).astype(f32)}
    a.update(points_bag(pts, descs))
    return a


class Fuse2Case:
    """Fuse(pKF, vpMapPoints, th, bRight), one call per side of the case ("left", "right").  The keyframe holds no map point at entry;
    the right pose is the reference's own (the stand-in's getters, from the left pose and Tlr)."""
    fn = "fuse2"
    exits = F2.EXITS

    def __init__(self, name, make, tags=()):
        self.name, self._make, self._a, self.tags = name, make, None, tuple(tags)

    def arrays(self):
        if self._a is None:
            self._a = self._make()
        return self._a

    @property
    def calls(self):
        a = load_fixture(self.name)[0] if os.path.exists(fixture_path(self.name)) else self.arrays()
        return ["right" if s else "left" for s in a["sides"]]

    def kf(self, a):
        return F2.KF2(a["kf_x"], a["kf_y"], a["kf_octave"], a["kf_desc"], int(a["kf_nleft"][0]), a["kf_pose"])

    def bounds(self, a):
        return F2.Bounds(*[f32(v) for v in a["bounds"]])

    def bag(self, a, call):
        right = call == "right"
        nmp, kf = int(a["nmp"][0]), self.kf(a)
        bag = {"fn": _fn("fuse2"), "params": _params(0.6, 1, a["th"][0], right), "list": np.arange(nmp, dtype=np.int32)}
        bag.update({key: v for key, v in a.items() if key.startswith("mp_")})
        bag["mp_in_kf"] = a["skip"][int(right)].reshape(1, nmp)
        b = a["bounds"]
        cam = np.array([0, 0, 0, 0, 0, b[0], b[1], b[2], b[3], 0], f32)
        pose = kf.pose[0]
        bag.update(table_bag("t0_", kf.x, kf.y, kf.octave, None, kf.desc, cam, R=pose[:9].reshape(3, 3), t=pose[9:12], Ow=pose[12:15],
                             nleft=a["kf_nleft"], kb1=a["kb1"], kb2=a["kb2"], Tlr=a["Tlr"]))
        return bag

    def _full(self, a, best):
        return (best,) + fuse_apply(best, np.full(len(a["kf_x"]), -1, np.int32), a["mp_bad"], a["mp_nobs"], False)

    def expected(self, a, call, res):
        """-> best_idx[nmp] (rows over the keyframe's N), the Replace / AddObservation / AddMapPoint calls in order, the keyframe's
        rows after them, (no vpReplacePoint), the return value"""
        nmp = int(a["nmp"][0])
        ops = res["ops"].reshape(-1, 3)
        return rows_from_ops(ops, nmp), ops[ops[:, 0] >= 3], res["kf_mp"], np.full(nmp, -1, np.int32), int(res["ret"][0])

    def restate(self, a, call, fast=False, exits=None, rules=F2.REF):
        right = call == "right"
        pts, descs = points_of(a, int(a["nmp"][0]))
        if fast:
            best = F2.fuse2_fast(pts, descs, self.kf(a), right, a["th"][0], a["skip"][int(right)], bounds=self.bounds(a))[0]
        else:
            best = F2.fuse2_scalar(pts, descs, self.kf(a), right, a["th"][0], a["skip"][int(right)], exits, rules, bounds=self.bounds(a))[0]
        return self._full(a, best)

    def undecided(self, a):
        pts, _ = points_of(a, int(a["nmp"][0]))
        return len(F2.examine(pts, [self.kf(a)], float(a["th"][0]), a["skip"][None], bounds=self.bounds(a))[1])

    def device(self, fe, a, calls):
        """{call: (the call's side out of ONE call with sides = 3, out of a call with that side alone)}"""
        pts, descs = points_of(a, int(a["nmp"][0]))
        kf = self.kf(a)
        kfs = [(keypoints(kf.x, kf.y, kf.octave), kf.desc, kf.nleft, kf.pose)]
        run = lambda sides: fe.fuse_search_two_cameras(pts, descs, kfs, a["kb1"], a["kb2"], tuple(float(v) for v in a["bounds"]), a["th"][0],
                                                       sides, a["skip"][None], FU.level_ratio())[0][0]
        both = run(3)
        return {c: (self._full(a, both[int(c == "right")]), self._full(a, run(2 if c == "right" else 1)[int(c == "right")])) for c in calls}


def _fuse2_hand(which):
    """Known answers of test_fuse_two_cameras_cpu.py, one case each (a keyframe at the origin, one point):
      axis      the point on the left optical axis: the left call finds row 0, the right call the right camera's row 0 as row 0 + NLeft
      tie       two right keypoints at equal distance across a cell border: the one visited first wins, returned as its row + NLeft
      radius    a keypoint exactly at the radius (th = 2) is outside the window
      behind    z < 0 in the camera, though KannalaBrandt8::project puts it inside the image: rejected by the depth gate (:1459)
      chi2      a keypoint 2.5 px away at octave 0: inside the window, rejected only by 6.25 > 5.99
      th_low    the only candidate at distance exactly TH_LOW: fused
      max_x     mnMaxX set to the projection's own u: u < mnMaxX fails, nothing is searched"""
    Z, one, kf2 = F2.Z32, F2.one_point, F2.kf2_of
    cam = np.asarray(F2.CAMS[0], f32)
    pose = F2.kf_pose(F2.P0)
    pts, descs, th, bounds, sides = one([0, 0, 3]), Z[None], 3.0, F2.BOUNDS, (0,)
    far = [(10.0, 10.0, Z), (20.0, 10.0, Z), (30.0, 10.0, Z)]
    if which == "axis":
        ur, vr = F2.project_side(pts, pose, True)
        kf, sides = kf2([(cam[2], cam[3], Z)], [(ur, vr, Z)]), (0, 1)
    elif which == "tie":
        pts = one([0, 0, 3], max_dist=6.0)
        u, v = (float(c) for c in F2.project_side(pts, pose, True))
        border = round((u - 4.0) / 8.0) * 8.0 + 4.0
        kf, sides = kf2([(10.0, 10.0, Z, 4)] * 3, [(border + 0.4, v, Z, 4), (border - 0.4, v, Z, 4)], pose), (1,)
    elif which == "radius":
        kf, th = kf2([(f32(cam[2] - f32(2.0)), cam[3], Z)], []), 2.0
    elif which == "behind":
        pos = np.array([0.7071, 0.7071, -0.2], f32) * f32(2.0)
        pts = one(pos)
        u, v = F2.oracle().kb8_project(cam, pos)
        kf = kf2([(u, v, Z)], [])
    elif which == "chi2":
        kf = kf2([(f32(cam[2] + f32(2.5)), cam[3], Z)] + far, [])
    elif which == "th_low":
        kf = kf2([(cam[2], cam[3], B2.desc_with_bits(50))] + far, [])
    elif which == "max_x":
        kf, bounds = kf2([(cam[2], cam[3], Z)], []), F2.Bounds(f32(0.0), f32(cam[2]), f32(0.0), f32(512.0))
    return fuse2_arrays(pts, descs, kf, None, th, bounds, sides)


FUSE2_HAND = {"axis": [[0], [1]], "tie": [[4]], "radius": [[-1]], "behind": [[-1]], "chi2": [[-1]], "th_low": [[0]], "max_x": [[-1]]}      # best_idx per call
FUSE2_SEEDS = ((71, 3.0), (72, 4.0))


def _fuse2_seeded(seed, th):
    c = F2.fuse2_case(seed, 1, nmp=300, nfeat=(220, 170))
    return fuse2_arrays(c.pts, c.descs, c.kfs[0], c.skip[0], th)


FUSE2_CASES = [Fuse2Case("fuse2_hand_" + w, (lambda w=w: _fuse2_hand(w)), tags=(w,)) for w in FUSE2_HAND] + \
              [Fuse2Case("fuse2_seed%d" % s, (lambda s=s, th=th: _fuse2_seeded(s, th))) for s, th in FUSE2_SEEDS]


# --------------------------------------------------------------- SearchByProjection(F, vpMapPoints, th, ...) with F.Nleft != -1
L2_BOUNDS = (0.0, 640.0, 0.0, 480.0)


def local2_arrays(kp_l, d_l, occ_l, l2r, kp_r, d_r, occ_r, r2l, track, track_r, qdesc, bad=None, th=1.0, far=False, th_far=50.0, nnratio=0.8,
                  bounds=L2_BOUNDS):
    """A frame of two cameras (keypoints x, y, octave per camera, descriptors, occ: 0 = NULL, 1 = a map point WITH observations;
    mvLeftToRightMatch / mvRightToLeftMatch) and the list's points: track[nq, 8] as the single-camera case has it (mbTrackInView,
    mTrackProjX, mTrackProjY, -, mTrackDepth, mnTrackScaleLevel, mTrackViewCos, -), track_r[nq, 6] = mbTrackInViewR, mTrackProjXR,
    mTrackProjYR, mnTrackScaleLevelR, mTrackViewCosR, mTrackDepthR.  Every list point has observations (it comes from a keyframe)."""
    nq = len(track)
    cat = lambda f: np.concatenate([kp_l[f], kp_r[f]])
    a = {"th": _params(th, far, th_far, nnratio), "bounds": np.array(bounds, f32), "cur_x": cat("x"), "cur_y": cat("y"), "cur_octave": cat("octave"),
         "cur_desc": np.concatenate([d_l, d_r]).astype(np.uint8).reshape(-1, 32), "cur_nleft": np.array([len(kp_l)], np.int32),
         "cur_occ": np.concatenate([occ_l, occ_r]).astype(np.uint8), "l2r": np.asarray(l2r, np.int32), "r2l": np.asarray(r2l, np.int32),
         "mp_track": np.asarray(track, f32).reshape(nq, 8), "mp_track_r": np.asarray(track_r, f32).reshape(nq, 6)}
    assert len(a["cur_x"]) <= MAX_ROWS and nq <= MAX_POINTS
    a.update(points_bag(np.zeros(nq, FU.FUSE_POINT_DT), qdesc, bad=np.zeros(nq, np.uint8) if bad is None else bad, nobs=np.ones(nq, np.int32)))
    return a


class Local2Case:
    """SearchByProjection(F, vpMapPoints, th, bFarPoints, thFarPoints) with F.Nleft != -1: one call.  The function projects nothing:
    the track fields ARE the queries, so the pin is the control flow of :44-214 alone."""
    fn = "local2"
    calls = ("call",)

    def __init__(self, name, make, tags=()):
        self.name, self._make, self._a, self.tags = name, make, None, tuple(tags)

    def arrays(self):
        if self._a is None:
            self._a = self._make()
        return self._a

    def queries(self, a):
        """:50-73 and :145-151: who takes part per camera, the radius (th multiplies the LEFT radius only), the level windows."""
        th, far, th_far = f32(a["th"][0]), bool(a["th"][1]), f32(a["th"][2])
        nq = len(a["mp_track"])
        ql, qr = np.zeros(nq, HM.PROJ_QUERY_DT), np.zeros(nq, HM.PROJ_QUERY_DT)
        for i, (t, tr) in enumerate(zip(a["mp_track"], a["mp_track_r"])):
            takes_part = not (far and t[4] > th_far) and not a["mp_bad"][i]
            r = f32(2.5) if float(t[6]) > 0.998 else f32(4.0)
            if float(th) != 1.0:
                r = f32(r * th)
            level = int(t[5])
            ql[i] = (t[1], t[2], f32(r * FU.SF[level]), 0, level - 1, level, 0, int(t[0] != 0 and takes_part))
            rr = f32(2.5) if float(tr[4]) > 0.998 else f32(4.0)
            lr = int(tr[3])
            qr[i] = (tr[1], tr[2], f32(rr * FU.SF[max(lr, 0)]), 0, lr - 1, lr, 0, int(tr[0] != 0 and lr != -1 and takes_part))
        return ql, qr, a["mp_desc"]

    def sides(self, a):
        nl = int(a["cur_nleft"][0])
        kp = keypoints(a["cur_x"], a["cur_y"], a["cur_octave"])
        occ = (a["cur_occ"] == 1).astype(np.uint8)
        return (kp[:nl], a["cur_desc"][:nl], occ[:nl]), (kp[nl:], a["cur_desc"][nl:], occ[nl:])

    def bag(self, a, call="call"):
        nq, occ = len(a["mp_track"]), a["cur_occ"]
        mp = np.full(len(occ), -1, np.int32)
        mp[occ != 0] = nq + np.arange(int((occ != 0).sum()))
        extra = extra_points(int((occ != 0).sum()), nobs=np.full(int((occ != 0).sum()), 3))
        b = a["bounds"]
        bag = {"fn": _fn("local2"), "params": _params(a["th"][3], 1, a["th"][0], a["th"][1], a["th"][2]), "list": np.arange(nq, dtype=np.int32)}
        bag.update(concat_points({k: v for k, v in a.items() if k.startswith("mp_") and not k.startswith("mp_track")}, extra))
        bag["mp_track"] = np.concatenate([a["mp_track"], np.zeros((len(extra["mp_bad"]), 8), f32)])
        bag["mp_track_r"] = np.concatenate([a["mp_track_r"], np.zeros((len(extra["mp_bad"]), 6), f32)])
        bag.update(table_bag("t0_", a["cur_x"], a["cur_y"], a["cur_octave"], None, a["cur_desc"], np.array([0, 0, 0, 0, 0, b[0], b[1], b[2], b[3], 0], f32),
                             mp=mp, nleft=a["cur_nleft"], kb1=np.asarray(T2.CAMS[0], f32), kb2=np.asarray(T2.CAMS[1], f32),
                             Tlr=np.hstack([T2.TLR_R, T2.TLR_T.reshape(3, 1)]).astype(f32), l2r=a["l2r"], r2l=a["r2l"]))
        return bag

    def expected(self, a, call, res):
        """-> the frame's Nleft + Nright slots that hold a list point after the call (-1: none, or what they held before), the return"""
        nq = len(a["mp_track"])
        rows = res["frame_mp"]
        return np.where(rows < nq, rows, -1).astype(np.int32), int(res["ret"][0])

    def _run(self, fn_, a, device):
        ql, qr, qd = self.queries(a)
        (kl, dl, ol), (kr, dr, orr) = self.sides(a)
        bounds = tuple(float(v) for v in a["bounds"])
        if device:
            n, mpl, mpr = fn_(ql, qr, qd, kl, dl, a["l2r"], kr, dr, a["r2l"], bounds, a["th"][3], ol, orr)
        else:
            n, mpl, mpr = fn_(ql, qr, qd, kl, dl, ol, a["l2r"], kr, dr, orr, a["r2l"], bounds, a["th"][3])
        return np.concatenate([mpl, mpr]).astype(np.int32), int(n)

    def oracle(self, po, a):
        return self._run(po.search_local_map_fisheye, a, False)

    def restate(self, a, call="call", exits=None, misread=()):
        """ORBmatcher.cc:44-214 with F.Nleft != -1 in Python, the reference's control flow (windows by helpers_matchers._area, the
        walking order of GetFeaturesInArea).  misread, the deliberate misreadings:
          right_after_left_ratio_fail   the left ratio failure does not leave the map point (:127 read as skipping the left only)
          left_empty_skips_right        an empty left window leaves the map point (:75 read as the `continue` of :153)
          th_on_right                   th multiplies the right radius too (:148 read as :67-70)
          no_partner_copy               mvLeftToRightMatch / mvRightToLeftMatch are not written (:132-136, :199-203)
          ratio_any_level               the ratio test without bestLevel == bestLevel2
          ratio_double                  bestDist > (double)mfNNratio * bestDist2
          right_slot_local              the right occupancy read at idx, not idx + Nleft (:169)
          th_high_strict                bestDist < TH_HIGH"""
        ex = exits if exits is not None else Counter()
        ql, qr, qd = self.queries(a)
        if "th_on_right" in misread and float(f32(a["th"][0])) != 1.0:
            qr = qr.copy(); qr["radius"] = (qr["radius"] * f32(a["th"][0])).astype(f32)
        (kl, dl, ol), (kr, dr, orr) = self.sides(a)
        bounds = tuple(float(v) for v in a["bounds"])
        nl = len(kl)
        taken = np.concatenate([ol, orr]) != 0
        slots = np.full(len(taken), -1, np.int32)
        ratio = float(f32(a["th"][3])) if "ratio_double" in misread else f32(a["th"][3])
        cells = (HM._cells(kl, bounds), HM._cells(kr, bounds))
        n = 0

        def best2(cam, Q, d):
            kp, desc, base = ((kl, dl, 0), (kr, dr, nl))[cam]
            px, py, ingrid, gw, gh = cells[cam]
            idx = HM._area(Q, kp, px, py, ingrid, bounds, gw, gh, [])
            if idx is None or idx.size == 0:
                return None
            bd, bl, bd2, bl2, bi = 256, -1, 256, -1, -1
            for i2 in idx.tolist():
                if taken[i2 + (0 if (cam and "right_slot_local" in misread) else base)]:
                    continue
                dist = int(HM.hamming(d[None], desc[i2:i2 + 1])[0])
                if dist < bd:
                    bd2, bd, bl2, bl, bi = bd, dist, bl, int(kp["octave"][i2]), i2
                elif dist < bd2:
                    bl2, bd2 = int(kp["octave"][i2]), dist
            return bd, bl, bd2, bl2, bi

        def fails_ratio(bd, bl, bd2, bl2):
            same = bl == bl2 or "ratio_any_level" in misread
            return same and (bd > ratio * bd2 if "ratio_double" in misread else f32(bd) > f32(ratio * f32(bd2)))

        side = lambda cam: "LR"[cam]
        for i in range(len(ql)):
            if not ql["valid"][i] and not qr["valid"][i]:
                ex["not_in_view"] += 1; continue
            if ql["valid"][i]:
                b = best2(0, ql[i], qd[i])
                if b is None:
                    ex["empty_window_L"] += 1
                    if "left_empty_skips_right" in misread:
                        continue
                else:
                    bd, bl, bd2, bl2, bi = b
                    if bd < 100 or (bd == 100 and "th_high_strict" not in misread):
                        if fails_ratio(bd, bl, bd2, bl2):
                            ex["ratio_failed_L"] += 1
                            if "right_after_left_ratio_fail" not in misread:
                                continue
                        else:
                            slots[bi] = i; taken[bi] = True; n += 1; ex["matched_L"] += 1
                            if a["l2r"][bi] != -1 and "no_partner_copy" not in misread:
                                slots[nl + a["l2r"][bi]] = i; taken[nl + a["l2r"][bi]] = True; n += 1; ex["copied_to_R"] += 1
                    else:
                        ex["no_candidate_L" if bi < 0 else "above_TH_HIGH_L"] += 1
            if qr["valid"][i]:
                b = best2(1, qr[i], qd[i])
                if b is None:
                    ex["empty_window_R"] += 1; continue
                bd, bl, bd2, bl2, bi = b
                if bd < 100 or (bd == 100 and "th_high_strict" not in misread):
                    if fails_ratio(bd, bl, bd2, bl2):
                        ex["ratio_failed_R"] += 1; continue
                    if a["r2l"][bi] != -1 and "no_partner_copy" not in misread:
                        slots[a["r2l"][bi]] = i; taken[a["r2l"][bi]] = True; n += 1; ex["copied_to_L"] += 1
                    slots[nl + bi] = i; taken[nl + bi] = True; n += 1; ex["matched_R"] += 1
                else:
                    ex["no_candidate_R" if bi < 0 else "above_TH_HIGH_R"] += 1
        return slots, n

    exits = ("not_in_view", "empty_window_L", "empty_window_R", "ratio_failed_L", "ratio_failed_R", "matched_L", "matched_R", "copied_to_R",
             "copied_to_L", "no_candidate_L", "no_candidate_R", "above_TH_HIGH_L", "above_TH_HIGH_R")
    misreadings = ("right_after_left_ratio_fail", "left_empty_skips_right", "th_on_right", "no_partner_copy", "ratio_any_level", "ratio_double",
                   "right_slot_local", "th_high_strict")

    def device(self, fe, a, calls):
        r = self._run(fe.search_local_map_fisheye, a, True)
        return {"call": (r, r)}


def _lattice(nslots):
    return [(20.0 + 40 * (s % 16), 20.0 + 40 * (s // 16)) for s in range(nslots)]


def _local2_hand(nnratio=0.8):
    """One list point per lattice site (40 px apart: the windows do not see each other), level 0, straight on (radius 2.5), its own
    descriptor; bits(k): the point's descriptor k bits away.  Sites, in list order:
      0  in view left only, one left keypoint            -> left slot
      1  in view right only                              -> right slot (+ Nleft)
      2  in view of both                                 -> both slots
      3  left match whose keypoint has a stereo partner  -> the partner's right slot too (:132-133)
      4  right match whose keypoint has a left partner   -> the partner's left slot too (:199-206)
      5  left best 40 / second 50, same level            -> 40 <= 0.8f * 50 passes (the boundary), right searched and matched
         (with mfNNratio = 0.7: 35 / 50, which passes in float and would fail in double)
      6  left best 41 / second 50, same level            -> fails, and its `continue` (:127) leaves the right camera unsearched
      7  right best 40 / second 50                       -> passes
      8  right best 41 / second 50                       -> fails
      9  right candidate whose slot holds an observed map point at entry, a farther free one -> the farther one
      10 left best 41 / second 50 on different levels    -> no ratio test
      11 left window empty, right keypoint               -> right matched (an empty LEFT window does not skip the right, :75)
      12 left distance exactly TH_HIGH = 100, right 101  -> left only"""
    rng = np.random.default_rng(5)
    sites = _lattice(13)
    on = 40 if nnratio == 0.8 else 35          # 40 <= 0.8f * 50 = 40.0000006; 35 <= (float)(0.7f * 50.f) = 35.f, but 35 > 0.7f * 50 in double
    qd = rng.integers(0, 256, (13, 32), dtype=np.uint8)
    L, R = [], []                                                    # (x, y, octave, desc, occ)
    key = lambda lst, s, bits, dx=0.0, octave=0, occ=0, off=0: lst.append((sites[s][0] + dx, sites[s][1], octave, B2_flip(qd[s], bits, off), occ)) or len(lst) - 1
    inl, inr = np.ones(13, bool), np.ones(13, bool)
    l2r_pairs = []
    key(L, 0, 3); inr[0] = False
    key(R, 1, 3); inl[1] = False
    key(L, 2, 3); key(R, 2, 4)
    a3 = key(L, 3, 3); b3 = key(R, 3, 150, dx=15.0); inr[3] = False; l2r_pairs.append((a3, b3))
    a4 = key(L, 4, 150, dx=15.0); b4 = key(R, 4, 3); inl[4] = False; l2r_pairs.append((a4, b4))
    key(L, 5, on); key(L, 5, 50, dx=1.0, off=60); key(R, 5, 3)
    key(L, 6, on + 1); key(L, 6, 50, dx=1.0, off=60); key(R, 6, 3)
    key(R, 7, on); key(R, 7, 50, dx=1.0, off=60); inl[7] = False
    key(R, 8, on + 1); key(R, 8, 50, dx=1.0, off=60); inl[8] = False
    key(R, 9, 2, occ=1); key(R, 9, 30, dx=1.0, off=60); inl[9] = False
    key(L, 10, 41); key(L, 10, 50, dx=1.0, octave=1, off=60); inr[10] = False
    key(R, 11, 3)
    key(L, 12, 100); key(R, 12, 101)
    def side(rows):
        kp = keypoints(np.array([r[0] for r in rows], f32), np.array([r[1] for r in rows], f32), np.array([r[2] for r in rows], np.int32))
        return kp, np.array([r[3] for r in rows], np.uint8), np.array([r[4] for r in rows], np.uint8)
    (kl, dl, ol), (kr, dr, orr) = side(L), side(R)
    l2r, r2l = np.full(len(L), -1, np.int32), np.full(len(R), -1, np.int32)
    for x, y in l2r_pairs:
        l2r[x], r2l[y] = y, x
    track = np.array([(inl[s], sites[s][0], sites[s][1], 0, 5.0, 1 if s == 10 else 0, 1.0, 0) for s in range(13)], f32)
    track_r = np.array([(inr[s], sites[s][0], sites[s][1], 0, 1.0, 5.0) for s in range(13)], f32)
    return local2_arrays(kl, dl, ol, l2r, kr, dr, orr, r2l, track, track_r, qd, nnratio=nnratio)


def B2_flip(desc, bits, offset=0):
    """desc with `bits` bits flipped, starting at bit `offset`."""
    out = np.array(desc, np.uint8).copy()
    for b in range(offset, offset + bits):
        out[(b % 256) >> 3] ^= np.uint8(1 << (b & 7))
    return out


# the frame's slots after the hand case: left rows then right rows, by the docstring above
def local2_hand_want(a):
    nl = int(a["cur_nleft"][0])
    want = np.full(len(a["cur_x"]), -1, np.int32)
    L = {0: 0, 1: 2, 2: 3, 3: 4, 4: 5, 8: 10, 10: 12}            # left row -> list point
    R = {0: 1, 1: 2, 2: 3, 3: 4, 4: 5, 6: 7, 11: 9, 12: 11}      # right row -> list point
    for r, p in L.items():
        want[r] = p
    for r, p in R.items():
        want[nl + r] = p
    return want, len(L) + len(R)


def _local2_seeded(seed, th, far, nnratio, nl=210, nr=180, nq=300):
    """Random keypoints of two cameras, list points thrown near keypoints of either camera with near descriptors, partners for a
    third of the keypoints, a fifth of the slots held at entry; levels, viewing cosines, depths and view flags at random."""
    rng = np.random.default_rng(seed)
    def camera(n):
        return keypoints(rng.uniform(0, 640, n).astype(f32), rng.uniform(0, 480, n).astype(f32), rng.integers(0, 4, n))
    kl, kr = camera(nl), camera(nr)
    dl, dr = rng.integers(0, 256, (nl, 32), dtype=np.uint8), rng.integers(0, 256, (nr, 32), dtype=np.uint8)
    for i in range(5, nl, 6):                                        # close pairs: second bests on the same spot
        kl["x"][i], kl["y"][i], kl["octave"][i], dl[i] = kl["x"][i - 1] + 1, kl["y"][i - 1], kl["octave"][i - 1], B2_flip(dl[i - 1], 4)
    for i in range(5, nr, 6):
        kr["x"][i], kr["y"][i], kr["octave"][i], dr[i] = kr["x"][i - 1] + 1, kr["y"][i - 1], kr["octave"][i - 1], B2_flip(dr[i - 1], 4)
    l2r, r2l = np.full(nl, -1, np.int32), np.full(nr, -1, np.int32)
    k = min(nl, nr) // 3
    for x, y in zip(rng.permutation(nl)[:k], rng.permutation(nr)[:k]):
        l2r[x], r2l[y] = y, x
    sl, sr = rng.integers(0, nl, nq), rng.integers(0, nr, nq)
    track, track_r = np.zeros((nq, 8), f32), np.zeros((nq, 6), f32)
    track[:, 0], track_r[:, 0] = rng.random(nq) < 0.75, rng.random(nq) < 0.75
    track[:, 1], track[:, 2] = kl["x"][sl] + rng.uniform(-3, 3, nq), kl["y"][sl] + rng.uniform(-3, 3, nq)
    track_r[:, 1], track_r[:, 2] = kr["x"][sr] + rng.uniform(-3, 3, nq), kr["y"][sr] + rng.uniform(-3, 3, nq)
    track[:, 4] = rng.uniform(1, 80, nq)
    track[:, 5] = np.clip(kl["octave"][sl] + rng.integers(0, 2, nq), 0, 7)
    track_r[:, 3] = np.where(rng.random(nq) < 0.05, -1, np.clip(kr["octave"][sr] + rng.integers(0, 2, nq), 0, 7))
    track[:, 6], track_r[:, 4] = rng.choice([0.9, 0.999], nq), rng.choice([0.9, 0.999], nq)
    pick = rng.random(nq) < 0.5
    qd = np.where(pick[:, None], dl[sl], dr[sr]).copy()
    for i in range(nq):
        qd[i] = B2_flip(qd[i], int(rng.integers(0, 45)), int(rng.integers(0, 200)))
    # the other camera sees the same thing: its keypoint near the point's projection gets a near descriptor too
    for i in np.nonzero(rng.random(nq) < 0.6)[0]:
        if pick[i]:
            dr[sr[i]] = B2_flip(qd[i], int(rng.integers(0, 40)), int(rng.integers(0, 200)))
        else:
            dl[sl[i]] = B2_flip(qd[i], int(rng.integers(0, 40)), int(rng.integers(0, 200)))
    return local2_arrays(kl, dl, rng.random(nl) < 0.2, l2r, kr, dr, rng.random(nr) < 0.2, r2l, track, track_r, qd, bad=rng.random(nq) < 0.05,
                         th=th, far=far, nnratio=nnratio)


LOCAL2_CASES = [Local2Case("local2_hand", _local2_hand, tags=("hand",)),
                Local2Case("local2_hand_ratio07", lambda: _local2_hand(0.7), tags=("hand",)),
                Local2Case("local2_seed1", lambda: _local2_seeded(1, 1.0, False, 0.8)),
                Local2Case("local2_seed2_th3_far", lambda: _local2_seeded(2, 3.0, True, 0.8)),
                Local2Case("local2_seed3_ratio07", lambda: _local2_seeded(3, 1.0, False, 0.7, nl=190, nr=200))]


# ---------------------------------------------------------- SearchByProjection(CurrentFrame, LastFrame, th, bMono), Nleft != -1
F2_MB = 0.5


def frame2_arrays(kp_l, d_l, occ_l, kp_r, d_r, occ_r, pos, qdesc, nobs, last_octave, last_angle, last_held=None, last_outlier=None, trl=(3.0, 0.0, 0.0),
                  last_tz=0.0, th=10.0, mono=False, check_ori=True, bounds=L2_BOUNDS):
    """The current frame of two cameras at the identity pose with the identity pinhole camera (u = x / z: exact for z = 1), Trl =
    [I | trl], so that the projections :2002 and :2084-2086 are exact in float and the pin is the control flow after them; the last
    frame (one camera) holds list point i in row i, at [I | (0, 0, last_tz)]: tlc.z = last_tz against mb = 0.5 decides forward /
    backward (:1981-1982).  occ: 0 = NULL, 1 = a map point WITH observations."""
    nq = len(pos)
    cat = lambda f: np.concatenate([kp_l[f], kp_r[f]])
    pts = np.zeros(nq, FU.FUSE_POINT_DT)
    pts["pos"] = pos
    a = {"th": _params(th, mono, check_ori), "bounds": np.array(bounds, f32), "cur_x": cat("x"), "cur_y": cat("y"), "cur_octave": cat("octave"),
         "cur_angle": cat("angle"), "cur_desc": np.concatenate([d_l, d_r]).astype(np.uint8).reshape(-1, 32), "cur_nleft": np.array([len(kp_l)], np.int32),
         "cur_occ": np.concatenate([occ_l, occ_r]).astype(np.uint8), "Trl": np.hstack([np.eye(3, dtype=f32), np.array(trl, f32).reshape(3, 1)]),
         "last_Tcw": mat44(np.concatenate([np.eye(3, dtype=f32).reshape(9), np.array([0, 0, last_tz], f32)])),
         "last_octave": np.asarray(last_octave, np.int32), "last_angle": np.asarray(last_angle, f32),
         "last_held": np.ones(nq, np.uint8) if last_held is None else np.asarray(last_held, np.uint8),
         "last_outlier": np.zeros(nq, np.uint8) if last_outlier is None else np.asarray(last_outlier, np.uint8)}
    assert len(a["cur_x"]) <= MAX_ROWS and nq <= MAX_POINTS
    a.update(points_bag(pts, qdesc, bad=np.zeros(nq, np.uint8), nobs=nobs))
    return a


def _walk(q, lists, dists, occ, ncur, allowed, th_high):
    """(test_two_camera_projection_cpu._walk with the threshold as a parameter)"""
    taken = np.zeros(ncur, bool) if occ is None else (np.asarray(occ) != 0).copy()
    raw = np.full(len(q), -1, np.int32)
    for i in np.flatnonzero(allowed):
        idx, d = lists[i], dists[i]
        free = ~taken[idx]
        if not free.any():
            continue
        k = int(np.argmin(np.where(free, d, 1 << 20)))
        if d[k] > th_high:
            continue
        raw[i] = idx[k]
        if not (q["valid"][i] & P2.NO_OBS):
            taken[idx[k]] = True
    return raw


class Frame2Case:
    """SearchByProjection(CurrentFrame, LastFrame, th, bMono) with CurrentFrame.Nleft != -1: one call."""
    fn = "frame2"
    calls = ("call",)
    misreadings = ("right_searched_whatever_the_left", "per_camera_histogram", "th_high_strict", "right_slot_local", "right_window_neutral")

    def __init__(self, name, make, tags=()):
        self.name, self._make, self._a, self.tags = name, make, None, tuple(tags)

    def arrays(self):
        if self._a is None:
            self._a = self._make()
        return self._a

    def queries(self, a):
        """:1971-2022 and :2084-2101: both projections of every point the last frame holds (x3Dr = Rrl * x3Dc + trl, one gemm), the
        window from its octave and the direction of motion, the same for both cameras."""
        th, mono = f32(a["th"][0]), bool(a["th"][1])
        tlc_z = a["last_Tcw"][2, 3]
        forward, backward = bool(tlc_z > f32(F2_MB)) and not mono, bool(-tlc_z > f32(F2_MB)) and not mono
        n = len(a["last_octave"])
        ql, qr = np.zeros(n, HM.PROJ_QUERY_DT), np.zeros(n, HM.PROJ_QUERY_DT)
        Trl = a["Trl"]
        with np.errstate(all="ignore"):
            for i in range(n):
                if not a["last_held"][i] or a["last_outlier"][i]:
                    continue
                p = a["mp_pos"][i]
                if f32(1.0 / f64(p[2])) < 0:
                    continue
                o = int(a["last_octave"][i])
                lo, hi = (o, -1) if forward else (0, o) if backward else (o - 1, o + 1)
                pr = [FU.gemm_row(Trl[r, :3], p, Trl[r, 3]) for r in range(3)]
                valid = 1 if a["mp_nobs"][i] > 0 else 3
                ql[i] = (f32(p[0] / p[2]), f32(p[1] / p[2]), f32(th * FU.SF[o]), 0, lo, hi, a["last_angle"][i], valid)
                qr[i] = (f32(pr[0] / pr[2]), f32(pr[1] / pr[2]), f32(th * FU.SF[o]), 0, lo, hi, 0, 0)
        return ql, qr, a["mp_desc"]

    def sides(self, a):
        nl = int(a["cur_nleft"][0])
        kp = keypoints(a["cur_x"], a["cur_y"], a["cur_octave"], a["cur_angle"])
        occ = (a["cur_occ"] == 1).astype(np.uint8)
        return (kp[:nl], a["cur_desc"][:nl], occ[:nl]), (kp[nl:], a["cur_desc"][nl:], occ[nl:])

    def bag(self, a, call="call"):
        nq, occ = len(a["last_octave"]), a["cur_occ"]
        mp = np.full(len(occ), -1, np.int32)
        mp[occ != 0] = nq + np.arange(int((occ != 0).sum()))
        extra = extra_points(int((occ != 0).sum()), nobs=np.full(int((occ != 0).sum()), 3))
        b = a["bounds"]
        cam = np.array([1, 1, 0, 0, 0, b[0], b[1], b[2], b[3], F2_MB], f32)
        bag = {"fn": _fn("frame2"), "params": _params(0.9, a["th"][2], a["th"][0], a["th"][1])}
        bag.update(concat_points({k: v for k, v in a.items() if k.startswith("mp_")}, extra))
        bag.update(table_bag("t0_", a["cur_x"], a["cur_y"], a["cur_octave"], a["cur_angle"], a["cur_desc"], cam, mp=mp, nleft=a["cur_nleft"],
                             kb1=np.asarray(T2.CAMS[0], f32), kb2=np.asarray(T2.CAMS[1], f32), pinhole=np.array([1, 1, 0, 0], f32),
                             Tlr=np.hstack([np.eye(3, dtype=f32), -a["Trl"][:, 3:]]).astype(f32), Trl=a["Trl"], Tcw=np.eye(4, dtype=f32)))
        z = np.zeros(nq, f32)
        bag.update(table_bag("t1_", z, z, a["last_octave"], a["last_angle"], np.zeros((nq, 32), np.uint8), cam,
                             mp=np.where(a["last_held"] != 0, np.arange(nq), -1).astype(np.int32), outlier=a["last_outlier"], Tcw=a["last_Tcw"]))
        return bag

    def expected(self, a, call, res):
        """-> the frame's Nleft + Nright slots that hold a list point after the call (-1: none, or what they held before), the return"""
        nq = len(a["last_octave"])
        rows = res["frame_mp"]
        return np.where(rows < nq, rows, -1).astype(np.int32), int(res["ret"][0])

    def _slots(self, a, out):
        n, bl, br, rl, rr = out[:5]
        (kl, _, _), (kr, _, _) = self.sides(a)
        return np.concatenate([rows_after(rl, bl, len(kl)), rows_after(rr, br, len(kr))]).astype(np.int32), int(n)

    def _args(self, a):
        ql, qr, qd = self.queries(a)
        (kl, dl, ol), (kr, dr, orr) = self.sides(a)
        return (ql, qr, qd, kl, dl, kr, dr, tuple(float(v) for v in a["bounds"]), bool(a["th"][2])), (ol, orr)

    def restate(self, a, call="call", fast=False, exits=None, misread=()):
        """test_two_camera_projection_cpu.two_camera_scalar / two_camera_fast on the queries; with misread, the closed form rebuilt here:
          right_searched_whatever_the_left   the left `continue`s (:2004-2007, :2024) do not close the right camera
          per_camera_histogram               one rotation histogram per camera
          th_high_strict                     bestDist < TH_HIGH
          right_slot_local                   the right occupancy read at i2, not i2 + Nleft (:2111)
          right_window_neutral               the right window always [octave - 1, octave + 1] (:2096-2101 read as :2022 only)"""
        args, (ol, orr) = self._args(a)
        if not misread:
            out = (P2.two_camera_fast if fast else P2.two_camera_scalar)(*args, ol, orr)
            if exits is not None and not fast:
                for left, right in out[5]:
                    exits[left[0] + "_L"] += 1; exits[right[0] + "_R"] += 1
                for bl, br, rl, rr in zip(out[1], out[2], out[3], out[4]):
                    exits["filtered_L"] += int(rl >= 0 and bl < 0); exits["filtered_R"] += int(rr >= 0 and br < 0)
            return self._slots(a, out)
        ql, qr, qd, kl, dl, kr, dr, bounds, ori = args
        qr = P2._right_queries(ql, qr)
        if "right_window_neutral" in misread:
            qr["min_level"], qr["max_level"] = a["last_octave"] - 1, a["last_octave"] + 1
        if "right_slot_local" in misread:
            orr = np.resize(ol, len(kr)) if len(ol) else orr
        th_high = HM.TH_HIGH - 1 if "th_high_strict" in misread else HM.TH_HIGH
        ll, dsl, left_open = P2._windows(ql, qd, kl, dl, bounds, True)
        lr, dsr, _ = P2._windows(qr, qd, kr, dr, bounds, False)
        raw_l = _walk(ql, ll, dsl, ol, len(kl), left_open, th_high)
        raw_r = _walk(qr, lr, dsr, orr, len(kr), (ql["valid"] != 0) if "right_searched_whatever_the_left" in misread else left_open, th_high)
        best_l, best_r = raw_l.copy(), raw_r.copy()
        if ori:
            bins_l = np.array([P2.rot_bin(ql["angle"][i], kl["angle"][b]) if b >= 0 else -1 for i, b in enumerate(raw_l)], np.int64)
            bins_r = np.array([P2.rot_bin(ql["angle"][i], kr["angle"][b]) if b >= 0 else -1 for i, b in enumerate(raw_r)], np.int64)
            hist = lambda *bs: [int(h) for h in np.bincount(np.concatenate([b[b >= 0] for b in bs]), minlength=HM.HISTO_LENGTH)]
            if "per_camera_histogram" in misread:
                best_l[~np.isin(bins_l, HM.three_maxima(hist(bins_l))[0])] = -1
                best_r[~np.isin(bins_r, HM.three_maxima(hist(bins_r))[0])] = -1
            else:
                keep = HM.three_maxima(hist(bins_l, bins_r))[0]
                best_l[~np.isin(bins_l, keep)] = -1
                best_r[~np.isin(bins_r, keep)] = -1
        return self._slots(a, (int((best_l >= 0).sum() + (best_r >= 0).sum()), best_l, best_r, raw_l, raw_r))

    def device(self, fe, a, calls):
        args, (ol, orr) = self._args(a)
        r = self._slots(a, fe.search_by_projection_two_cameras(*args, ol, orr, with_raw=True))
        return {"call": (r, r)}


def _frame2_hand(last_tz=0.0, check_ori=True):
    """Rows on a 40 px lattice, th = 10 (radius 10 at octave 0), the right projection 3 px right of the left one; mnMinX = 10.
    bits(k): the row's descriptor k bits away.  Rows of the last frame, in order (docstring of the test works the slots out):
      0      a keypoint in both cameras                                   -> both slots (the right one at bestIdx2 + Nleft)
      1      left projection at u = 8.5 < mnMinX, a right keypoint at 11.5 -> nothing: the gate's `continue` leaves the right unsearched
      2      no left keypoint, a right one                                -> nothing: the empty left window does the same (:2024)
      3      the only left keypoint holds an observed map point, a right keypoint -> the right slot only
      4      right: the nearest keypoint's slot (i2 + Nleft) holds an observed map point, a farther one is free -> the farther one
      5      left 100 bits away, right 101                                -> left only (TH_HIGH is inclusive)
      6      left 101, right 100                                          -> right only
      7      last octave 2; right keypoints of octaves 0, 1, 3, 4, 2 at 1, 2, 4, 6, 8 bits -> neutral: octave 1; forward: 3; backward: 0
      8-12   five left-only matches turned by 30 degrees (bin 1)
      13-17  five right-only matches (left keypoint 150 bits away) turned by 60 (bin 2)
      18-19  two left-only matches turned by 90 (bin 3): third in the left camera's own histogram, fourth in the joint one -> removed
      20-21  two right-only matches turned by 120 (bin 4): the same on the right -> removed"""
    rng = np.random.default_rng(9)
    n = 22
    sites = _lattice(n)
    qd = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    pos = np.array([(x, y, 1.0) for x, y in sites], f32)
    pos[1] = (8.5, 140.0, 1.0)
    octave, angle = np.zeros(n, np.int32), np.zeros(n, f32)
    octave[7] = 2
    angle[8:13], angle[13:18], angle[18:20], angle[20:22] = 30.0, 60.0, 90.0, 120.0
    L, R = [], []
    def key(lst, s, bits, dx=0.0, octave=0, occ=0, off=0):
        lst.append((pos[s][0] + dx + (3.0 if lst is R else 0.0), pos[s][1], octave, qd_flip(qd[s], bits, off), occ))
    qd_flip = B2_flip
    key(L, 0, 2); key(R, 0, 4)
    key(R, 1, 2)
    key(R, 2, 2)
    key(L, 3, 2, occ=1); key(R, 3, 3)
    key(L, 4, 2); key(R, 4, 2, occ=1); key(R, 4, 30, dx=1.0, off=60)
    key(L, 5, 100); key(R, 5, 101)
    key(L, 6, 101); key(R, 6, 100)
    key(L, 7, 3, octave=2)
    for k, (o, bits) in enumerate(((0, 1), (1, 2), (3, 4), (4, 6), (2, 8))):
        key(R, 7, bits, dx=k - 2.0, octave=o, off=20 * k)
    for s in range(8, 13):
        key(L, s, 2)
    for s in range(13, 18):
        key(L, s, 150); key(R, s, 2)
    for s in (18, 19):
        key(L, s, 2)
    for s in (20, 21):
        key(L, s, 150); key(R, s, 2)
    def side(rows):
        kp = keypoints(np.array([r[0] for r in rows], f32), np.array([r[1] for r in rows], f32), np.array([r[2] for r in rows], np.int32), np.zeros(len(rows), f32))
        return kp, np.array([r[3] for r in rows], np.uint8), np.array([r[4] for r in rows], np.uint8)
    (kl, dl, ol), (kr, dr, orr) = side(L), side(R)
    return frame2_arrays(kl, dl, ol, kr, dr, orr, pos, qd, np.ones(n, np.int32), octave, angle, last_tz=last_tz, check_ori=check_ori,
                         bounds=(10.0, 640.0, 0.0, 480.0))


def frame2_hand_want(a):
    """The slots of _frame2_hand by its docstring (left rows then right rows; list point per slot)."""
    tz, ori = float(a["last_Tcw"][2, 3]), bool(a["th"][2])
    nl = int(a["cur_nleft"][0])
    want = np.full(len(a["cur_x"]), -1, np.int32)
    # left rows: 0:p0 1:p3(occ) 2:p4 3:p5 4:p6 5:p7 6-10:p8-12 11-15:p13-17 16,17:p18,19 18,19:p20,21
    left = {0: 0, 2: 4, 3: 5, 5: 7}
    left.update({6 + k: 8 + k for k in range(5)})
    if not ori:
        left.update({16: 18, 17: 19})
    # right rows: 0:p0 1:p1 2:p2 3:p3 4,5:p4 6:p5 7:p6 8-12:p7 (octaves 0 1 3 4 2) 13-17:p13-17 18,19:p20,21
    right = {0: 0, 3: 3, 5: 4, 7: 6, (10 if tz > 0.5 else 8 if tz < -0.5 else 9): 7}
    right.update({13 + k: 13 + k for k in range(5)})
    if not ori:
        right.update({18: 20, 19: 21})
    for r, p in left.items():
        want[r] = p
    for r, p in right.items():
        want[nl + r] = p
    return want, len(left) + len(right)


def _frame2_seeded(seed, last_tz, mono=False, nl=210, nr=180, nq=300):
    rng = np.random.default_rng(seed)
    def camera(n):
        return keypoints(rng.uniform(12, 640, n).astype(f32), rng.uniform(0, 480, n).astype(f32), rng.integers(0, 4, n), rng.uniform(0, 360, n).astype(f32))
    kl, kr = camera(nl), camera(nr)
    dl, dr = rng.integers(0, 256, (nl, 32), dtype=np.uint8), rng.integers(0, 256, (nr, 32), dtype=np.uint8)
    sl, sr = rng.integers(0, nl, nq), rng.integers(0, nr, nq)
    near_left = rng.random(nq) < 0.6
    pos = np.ones((nq, 3), f32)
    pos[:, 0] = np.where(near_left, kl["x"][sl], kr["x"][sr] - 3.0) + rng.uniform(-4, 4, nq)
    pos[:, 1] = np.where(near_left, kl["y"][sl], kr["y"][sr]) + rng.uniform(-4, 4, nq)
    pos[rng.random(nq) < 0.04, 0] = 5.0                              # left of mnMinX = 10
    behind = rng.random(nq) < 0.03
    pos[behind] *= -1.0                                              # invzc < 0
    qd = np.where(near_left[:, None], dl[sl], dr[sr]).copy()
    for i in range(nq):
        qd[i] = B2_flip(qd[i], int(rng.integers(0, 60)), int(rng.integers(0, 190)))
    for i in np.nonzero(rng.random(nq) < 0.7)[0]:                    # the other camera sees it too: a keypoint at its projection
        if near_left[i]:
            j = sr[i]; kr["x"][j], kr["y"][j], dr[j] = pos[i, 0] + 3.0 + rng.uniform(-2, 2), pos[i, 1] + rng.uniform(-2, 2), B2_flip(qd[i], int(rng.integers(0, 60)), 30)
        else:
            j = sl[i]; kl["x"][j], kl["y"][j], dl[j] = pos[i, 0] + rng.uniform(-2, 2), pos[i, 1] + rng.uniform(-2, 2), B2_flip(qd[i], int(rng.integers(0, 60)), 30)
    octave = np.where(near_left, kl["octave"][sl], kr["octave"][sr]) + rng.integers(-1, 2, nq)
    angle = (np.where(near_left, kl["angle"][sl], kr["angle"][sr]) + rng.choice([0.0, 0.0, 0.0, 0.0, 90.0, 200.0], nq)).astype(f32) % 360
    return frame2_arrays(kl, dl, rng.random(nl) < 0.2, kr, dr, rng.random(nr) < 0.2, pos, qd, np.where(rng.random(nq) < 0.85, 2, 0), np.clip(octave, 0, 7), angle,
                         last_held=rng.random(nq) < 0.95, last_outlier=rng.random(nq) < 0.03, last_tz=last_tz, mono=mono, bounds=(10.0, 640.0, 0.0, 480.0))


FRAME2_CASES = [Frame2Case("frame2_hand", _frame2_hand, tags=("hand",)),
                Frame2Case("frame2_hand_forward", lambda: _frame2_hand(1.0), tags=("hand",)),
                Frame2Case("frame2_hand_backward", lambda: _frame2_hand(-1.0), tags=("hand",)),
                Frame2Case("frame2_hand_no_orientation", lambda: _frame2_hand(0.0, False), tags=("hand",)),
                Frame2Case("frame2_seed1", lambda: _frame2_seeded(1, 0.0)),
                Frame2Case("frame2_seed2_forward", lambda: _frame2_seeded(2, 1.0)),
                Frame2Case("frame2_seed3_backward", lambda: _frame2_seeded(3, -1.0)),
                Frame2Case("frame2_seed4_mono", lambda: _frame2_seeded(4, 1.0, mono=True))]
CASES = KB8_CASES + TRI2_CASES + BOW2_CASES + FUSE2_CASES + LOCAL2_CASES + FRAME2_CASES
BY_NAME = {c.name: c for c in CASES}


def generate():
    """Runs oracle/_ref/pli_ref_match over every case and records inputs and outputs (not a test)."""
    total = 0
    assert set(FUNCTIONS) <= ref_functions(), "oracle/_ref/pli_ref_match is absent or lacks the two-camera functions: make -C oracle ref_match"
    os.makedirs(GOLD_DIR, exist_ok=True)
    for stale in sorted(set(os.listdir(GOLD_DIR)) - {c.name + ".npz" for c in CASES}):
        os.remove(os.path.join(GOLD_DIR, stale))
    for c in CASES:
        a = c.arrays()
        if c.fn == "tri2" or (c.fn == "fuse2" and not c.tags):              # (the hand cases of fuse2 sit ON their thresholds, in exact arithmetic)
            assert c.undecided(a) == 0, c.name
        save_fixture(c.name, a, {call: run_reference(c.bag(a, call)) for call in c.calls})
        size = os.path.getsize(fixture_path(c.name))
        total += size
        print("%-24s %-5s %3d calls %7d bytes" % (c.name, c.fn, len(c.calls), size))
    print("total %d bytes in %d files" % (total, len(CASES)))
    assert total <= SIZE_CAP, total
    _FIX.clear()


# ---------------------------------------------------------------------- KannalaBrandt8 in float32, the libm results handed in
def ulp_step(x, k):
    """The float32 k steps after x (k = -1, 0, 1)."""
    x = f32(x)
    return x if k == 0 else np.nextafter(x, f32(np.inf) if k > 0 else f32(-np.inf))


def rounded(fn, *args):
    """A libm function of float32 arguments, correctly rounded for every purpose here: evaluated in double, rounded once."""
    return f32(fn(*[float(f32(v)) for v in args]))


def project32(cam, p, dtheta=0, dpsi=0):
    """KannalaBrandt8::project (KannalaBrandt8.cpp:28-42) in float32: atan2f correctly rounded and then moved dtheta / dpsi floats;
    the two products with cos / sin and the sums with cx / cy in double, as the compiled reference has them (it imports sincos,
    not sincosf).  -> (u, v), (sqrtf(x2_plus_y2), z), (y, x): the outputs and the two argument pairs of atan2f."""
    fx, fy, cx, cy, k0, k1, k2, k3 = [f32(c) for c in cam]
    x, y, z = [f32(v) for v in p]
    rho = f32(np.sqrt(f32(f32(x * x) + f32(y * y))))
    theta = ulp_step(rounded(math.atan2, rho, z), dtheta)
    psi = ulp_step(rounded(math.atan2, y, x), dpsi)
    t2 = f32(theta * theta); t3 = f32(theta * t2); t5 = f32(t3 * t2); t7 = f32(t5 * t2); t9 = f32(t7 * t2)
    r = f32(f32(f32(f32(theta + f32(k0 * t3)) + f32(k1 * t5)) + f32(k2 * t7)) + f32(k3 * t9))
    u = f32(float(f32(fx * r)) * math.cos(float(psi)) + float(cx))
    v = f32(float(f32(fy * r)) * math.sin(float(psi)) + float(cy))
    return (u, v), (rho, z), (y, x)


def unproject32(cam, px, dtan=0):
    """KannalaBrandt8::unproject (:103-130) in float32: tanf correctly rounded and then moved dtan floats.
    -> ray (3 floats), theta handed to tanf (None when theta_d <= 1e-8), Newton steps taken."""
    fx, fy, cx, cy, k0, k1, k2, k3 = [f32(c) for c in cam]
    one = f32(1)
    with np.errstate(all="ignore"):
        pwx, pwy = f32(f32(f32(px[0]) - cx) / fx), f32(f32(f32(px[1]) - cy) / fy)
        theta_d = f32(np.sqrt(f32(f32(pwx * pwx) + f32(pwy * pwy))))
        theta_d = min(max(f32(-math.pi / 2), theta_d), f32(math.pi / 2))
        if not float(theta_d) > 1e-8:
            return (f32(pwx * one), f32(pwy * one), one), None, 0
        theta, steps = theta_d, 0
        for _ in range(10):
            t2 = f32(theta * theta); t4 = f32(t2 * t2); t6 = f32(t4 * t2); t8 = f32(t4 * t4)
            a, b, c, d = f32(k0 * t2), f32(k1 * t4), f32(k2 * t6), f32(k3 * t8)
            num = f32(f32(theta * f32(f32(f32(f32(one + a) + b) + c) + d)) - theta_d)
            den = f32(f32(f32(f32(one + f32(f32(3) * a)) + f32(f32(5) * b)) + f32(f32(7) * c)) + f32(f32(9) * d))
            fix = f32(num / den)
            theta = f32(theta - fix)
            steps += 1
            if abs(fix) < f32(1e-6):
                break
        scale = f32(ulp_step(rounded(math.tan, theta), dtan) / theta_d)
        return (f32(pwx * scale), f32(pwy * scale), one), theta, steps


def _bits(t):
    return np.array(t, f32).tobytes()


def explain_project(cam, p, recorded):
    """(dtheta, dpsi): by how many floats the reference's two atan2f results differ from the correctly rounded ones, found by
    asking which of the nine candidates gives the recorded pixel; (0, 0) comes first.  None: no candidate does."""
    for d in ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1)):
        if _bits(project32(cam, p, *d)[0]) == np.asarray(recorded, f32).tobytes():
            return d
    return None


def explain_unproject(cam, px, recorded):
    """dtan: by how many floats the reference's tanf result differs from the correctly rounded one (0 first); None: unexplained."""
    for d in (0, -1, 1):
        if _bits(unproject32(cam, px, d)[0]) == np.asarray(recorded, f32).tobytes():
            return d
    return None


def tri_expected(res):
    """(depth, p3d) as Frame::ComputeStereoFishEyeMatches stores them from the recorded TriangulateMatches outputs (Frame.cc:1609:
    kept when the return value is above 0.0001f; else -1 and zeros)."""
    ret = res["tri_ret"]
    keep = ret > f32(0.0001)
    return np.where(keep, ret, f32(-1)).astype(f32), np.where(keep[:, None], res["tri_p3d"], f32(0)).astype(f32)


def tri_residue(a, res):
    """Per pair: True where the reference's tanf, in the unprojection of kp1 by camera 1 or of kp2 by camera 2, is not the correctly
    rounded value (the ray it recorded is the one a tanf one float off gives).  p3D depends on libm through these two calls only;
    the atan2f of the two reprojections feeds gates, which every pair passes or fails with margin.  Raises on a ray that neither
    the correctly rounded tanf nor one a float off explains."""
    out = np.zeros(len(a["kp1"]), bool)
    for i in range(len(out)):
        d1 = explain_unproject(a["cam1"], a["kp1"][i], res["tri_r1"][i])
        d2 = explain_unproject(a["cam2"], a["kp2"][i], res["tri_r2"][i])
        assert d1 is not None and d2 is not None, (i, d1, d2)
        out[i] = d1 != 0 or d2 != 0
    return out


if __name__ == "__main__":
    import sys
    sys.path.insert(0, ROOT)                                                 # (the restatements load the oracle's binding from the package root)
    generate()
