"""ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo, bCoarse) (ORBmatcher.cc:965-1206), the branch
pKF1->mpCamera2 && pKF2->mpCamera2 (a rig of two KannalaBrandt8 cameras, NLeft != -1), restated in Python: the checker of
pli_search_for_triangulation_two_cameras (tests/test_triangulation_two_cameras_gpu.py, tests/test_cpp_triangulation_two_cameras.py).
Here, without a device: the scalar restatement (the reference's control flow) against a closed form (the minimum of the key
(dist << 32) | (0xffffffff - idx2) per idx1), a constructed corpus whose every pair that reaches the gate is decided, the exits of
the loops counted over it, hand-worked known answers, the mutations the corpus tells apart, and a build of the C++ harness.

What the branch reads (:1041-1132): a keyframe's N = NLeft + NRight features, the left camera's first; the keypoint of idx is
mvKeys[idx] / mvKeysRight[idx - NLeft]; bStereo1 / bStereo2 are false, so bOnlyStereo matches nothing and the epipole gate is
skipped; (bRight1, bRight2) picks one of the four relative poses of :995-1003 and the two cameras on every candidate; the gate is
KannalaBrandt8::epipolarConstrain = TriangulateMatches(...) > 0.0001f.  The gate of both restatements is
helpers_geometry.fisheye_expect (float64, written from the reference's text) with d0 = 0, d1 = 256, label "ok" = the gate passes.

The four relative poses are computed here in float32, one gemm per product (products and sum in double, one rounding), as
tests/stubs/opencv2/core/core.hpp evaluates the reference's cv::Mat expressions and test_fuse_search_cpu.gemm_row restates them.

Decided margins.  helpers_geometry.FISHEYE_MARGIN was measured on stereo rigs with a 0.1 m baseline.  For the relative poses of
this corpus (0.3 - 0.5 m between keyframes, the 0.1 m / 2 degree rig inside, one neighbour turned by 80 degrees) the same
deviations are measured here, oracle (pyoracle.stereo_fisheye / kb8_unproject / kb8_project: float32 in the reference's operation
order) against float64, on every pair of the corpus that reaches the gate, again on every run (test_margins_...):

  cosParallaxRays        worst 2.12e-7 (MEASURED_COS = 2.5e-7; 8.98e-8 on the stereo rigs: the rays of the turned neighbour are
                         longer), decided margin 8 x = 2e-6
  reprojection           worst 5.75e-5 px (MEASURED_REPROJ_PX = 7e-5); decided margin FISHEYE_MARGIN's 2e-3 px, the wider one
  depth, p3d             worst c in |diff| <= c 2^-23 max(1, z^2 / |t12|): 11.4 (MEASURED_C default = 13; 5.2 on the stereo rigs),
                         decided margin of z1, z2 and the depth floor 8 x = 104 units; a pair with a keypoint more than 1.1 rad
                         off its axis ("corner") 14.3 (MEASURED_C corner = 16), decided margin FISHEYE_MARGIN's 376 units

1803 pairs reach the gate.  The decided margin of a gate is 8 x its worst (the rule of helpers_geometry.py), and not below
FISHEYE_MARGIN.  The builder draws a keypoint whose pair comes out undecided again, as part of the draw; tables refused: 0,
undecided pairs: 0, keypoints drawn again: 0 for the committed seeds (asserted, printed).
"""
import math
import os
import subprocess
from collections import Counter, namedtuple
from dataclasses import dataclass, replace

import numpy as np
import pytest

import helpers_geometry as hg
from test_bow_search_cpu import POP8, desc_with_bits, distance, feature_vector, rot_bin, three_maxima

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TH_LOW, HISTO_LENGTH = 50, 30
f32, f64 = np.float32, np.float64
NLEVELS = 8
SIGMA2 = hg.fisheye_sigma2(NLEVELS, 1.2)                  # mvLevelSigma2
SCALE = np.sqrt(SIGMA2.astype(f64))                       # (the epipole-gate mutation only)
CAMS = (hg.TUMVI_KB8[0], hg.TUMVI_KB8[1])                 # mpCamera, mpCamera2
TLR_R, TLR_T = hg._roty(2.0).astype(f32), np.array([0.101, 0.002, -0.001], f32)      # mTlr

# ---- measured on the CPU against the oracle (see the docstring; test_margins_... measures them again and prints them) ----
MEASURED_COS = 2.5e-7
MEASURED_REPROJ_PX = 7.0e-5
MEASURED_C = {"default": 13.0, "corner": 16.0}
MARGIN = {"cos": max(8 * MEASURED_COS, hg.FISHEYE_MARGIN["cos"]), "px": max(8 * MEASURED_REPROJ_PX, hg.FISHEYE_MARGIN["px"]),
          "z_c": {k: max(8 * v, hg.FISHEYE_MARGIN["z_c"][k]) for k, v in MEASURED_C.items()}}
CORNER_RAD = 1.1

# one keyframe's tables: mvKeys then mvKeysRight (pt.x, pt.y, octave, angle), mDescriptors, the FeatureVector node that lists a
# feature (-1: none), GetMapPoint(i) != nullptr, NLeft
Table = namedtuple("Table", "x y octave angle desc node has_mp nleft")
# one neighbour of a call: its table, the four relative poses (4 x 12: ll, lr, rl, rr; R12 row major, then t12) and the epipole
# pKF2->mpCamera->project(R2w * Cw + t2w) (read by a mutation only)
Neighbour = namedtuple("Neighbour", "t2 rel ep")


def make_table(rows, nleft):
    """rows: (x, y, octave, angle, desc, node[, has_mp]) per feature, the left camera's first."""
    g = lambda i, dt, dflt=None: np.array([r[i] if len(r) > i else dflt for r in rows], dt)
    return Table(g(0, f32), g(1, f32), g(2, np.int32), g(3, f32), np.array([r[4] for r in rows], np.uint8).reshape(-1, 32),
                 g(5, np.int32), g(6, np.uint8, 0), int(nleft))


# ---- the host arithmetic of :995-1003 and KeyFrame.cc:1354-1373 ------------------------------------------------------------------

def gemm(A, B, alpha=1.0, C=None):
    """One CV_32F gemm: the float products and the sum in double, (float)(alpha * sum + C)."""
    A, B = np.asarray(A, f32), np.asarray(B, f32)
    if B.ndim == 1:
        B = B.reshape(-1, 1)
    out = np.zeros((A.shape[0], B.shape[1]), f32)
    for i in range(A.shape[0]):
        for j in range(B.shape[1]):
            d = 0.0
            for k in range(A.shape[1]):
                d += float(A[i, k]) * float(B[k, j])
            out[i, j] = f32(alpha * d + (float(np.asarray(C, f32).reshape(out.shape)[i, j]) if C is not None else 0.0))
    return out


class Pose:
    """Tcw of a keyframe (float32) and the four getters."""

    def __init__(self, Rcw, tcw):
        self.R, self.t = np.asarray(Rcw, f32).reshape(3, 3), np.asarray(tcw, f32).reshape(3, 1)

    def right_rotation(self):                         # Rrl * Rlw
        return gemm(TLR_R.T, self.R)

    def right_translation(self):                      # Rrl * tlw + trl, trl = -Rrl * tlr
        trl = gemm(TLR_R.T, TLR_T, -1.0)
        return gemm(TLR_R.T, self.t, 1.0, trl)

    def side(self, right):
        return (self.right_rotation(), self.right_translation()) if right else (self.R, self.t)

    def centre(self):                                 # Ow = -Rwc * tcw
        return gemm(self.R.T, self.t, -1.0)


def relative_poses(p1, p2):
    """rel[4, 12]: R12 = Ra * Rb.t(), t12 = Ra * (-Rb.t() * tb) + ta for (a, b) = ll, lr, rl, rr."""
    rel = np.zeros((4, 12), f32)
    for r1 in (0, 1):
        Ra, ta = p1.side(r1)
        for r2 in (0, 1):
            Rb, tb = p2.side(r2)
            rel[2 * r1 + r2, :9] = gemm(Ra, Rb.T).reshape(9)
            rel[2 * r1 + r2, 9:] = gemm(Ra, gemm(Rb.T, tb, -1.0), 1.0, ta).reshape(3)
    return rel


def epipole(p1, p2):
    C2 = gemm(p2.R, p1.centre(), 1.0, p2.t).reshape(3).astype(f64)
    return hg.kb8_project64(CAMS[0], C2)


def pose_from(rx, ry, rz, centre):
    R = hg._rot(rx, ry, rz)
    return Pose(R.astype(f32), (-R @ np.asarray(centre, f64)).astype(f32))


# ---- the gate ----------------------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class TriRules:
    rl_for_lr: bool = False               # Rrl / trl where (bRight1, bRight2) = (false, true) asks for Rlr / tlr, and the reverse
    wrong_camera: bool = False            # mpCamera for a right feature and mpCamera2 for a left one
    swap_sigmas: bool = False             # mvLevelSigma2 of kp2's octave for kp1 and the reverse
    first_wins: bool = False              # `dist < bestDist`: of equal distances the first listed stays
    epipole_gate: bool = False            # :1089-1097 applied although mpCamera2 is set


REF = TriRules()


def undecided(mg, corner):
    for k, v in mg.items():
        if k[0] == "_":
            continue
        lim = MARGIN["cos"] if k == "cos" else MARGIN["px"] if k in ("chi1", "chi2") else MARGIN["z_c"]["corner" if corner else "default"]
        if v < lim:
            return True
    return False


def off_axis(cam, x, y):
    return math.hypot((float(x) - float(f32(cam[2]))) / float(f32(cam[0])), (float(y) - float(f32(cam[3]))) / float(f32(cam[1])))


class Gate:
    """pCamera1->epipolarConstrain(pCamera2, kp1, kp2, R12, t12, sigma2[kp1.octave], sigma2[kp2.octave]) of one (pKF1, pKF2) in
    float64, remembered per pair: label, margins, undecided."""

    def __init__(self, t1, nb, rules=REF):
        self.t1, self.t2, self.rel, self.ep, self.rules, self.seen = t1, nb.t2, np.asarray(nb.rel, f32).reshape(4, 12), nb.ep, rules, {}

    def look(self, i1, i2):
        if (i1, i2) not in self.seen:
            t1, t2, ru = self.t1, self.t2, self.rules
            r1, r2 = int(i1 >= t1.nleft), int(i2 >= t2.nleft)
            which = 2 * r1 + r2
            if ru.rl_for_lr and which in (1, 2):
                which = 3 - which
            camA, camB = (CAMS[1 - r1], CAMS[1 - r2]) if ru.wrong_camera else (CAMS[r1], CAMS[r2])
            lab, mg, _ = hg.fisheye_expect((t1.x[i1], t1.y[i1], t1.octave[i1]), (t2.x[i2], t2.y[i2], t2.octave[i2]), camA, camB,
                                           self.rel[which, :9], self.rel[which, 9:], SIGMA2,
                                           rules=replace(hg.FREF, swap_sigmas=ru.swap_sigmas))
            corner = max(off_axis(camA, t1.x[i1], t1.y[i1]), off_axis(camB, t2.x[i2], t2.y[i2])) > CORNER_RAD
            self.seen[(i1, i2)] = (lab, mg, undecided(mg, corner), corner)
        return self.seen[(i1, i2)]

    def __call__(self, i1, i2):
        return self.look(i1, i2)[0] == "ok"

    def near_epipole(self, i2):           # :1091-1093 (the mutation)
        ex, ey = float(self.ep[0]) - float(self.t2.x[i2]), float(self.ep[1]) - float(self.t2.y[i2])
        return ex * ex + ey * ey < 100 * SCALE[self.t2.octave[i2]]


# ---- the two restatements ---------------------------------------------------------------------------------------------------

def search_scalar(t1, nb, only_stereo=False, coarse=False, check_orientation=False, exits=None, gate=None):
    """The reference's control flow, scalar: (vMatches12[n1] after the rotation filter, nmatches)."""
    ex = exits if exits is not None else Counter()
    gate = gate or Gate(t1, nb)
    ru, t2 = gate.rules, nb.t2
    n1 = len(t1.node)
    fv1, fv2 = feature_vector(t1.node), feature_vector(t2.node)
    keys1, keys2 = sorted(fv1), sorted(fv2)
    nmatches, matches12 = 0, [-1] * n1
    rot_hist = [[] for _ in range(HISTO_LENGTH)]
    i = j = 0
    while i < len(keys1) and j < len(keys2):
        if keys1[i] == keys2[j]:
            ex["node_common"] += 1
            for idx1 in fv1[keys1[i]]:
                if t1.has_mp[idx1]:
                    ex["has_mp1"] += 1
                    continue
                if only_stereo:                       # bStereo1 = (!pKF1->mpCamera2 && ...) = false
                    ex["only_stereo1"] += 1
                    continue
                best_dist, best_idx2, turned_away = TH_LOW, -1, 256
                for idx2 in fv2[keys2[j]]:
                    if t2.has_mp[idx2]:               # (vbMatched2 is never set)
                        ex["has_mp2"] += 1
                        continue
                    dist = distance(t1.desc[idx1], t2.desc[idx2])
                    if dist > TH_LOW or (dist >= best_dist and best_idx2 >= 0 if ru.first_wins else dist > best_dist):
                        ex["th_low" if dist > TH_LOW else "worse_than_best"] += 1
                        continue
                    if ru.epipole_gate and gate.near_epipole(idx2):
                        continue
                    if gate(idx1, idx2) or coarse:
                        ex["replaced" if best_idx2 >= 0 else "taken"] += 1
                        if dist == best_dist and best_idx2 >= 0:
                            ex["tie_later_wins"] += 1
                        best_idx2, best_dist = idx2, dist
                    else:
                        ex["gate_" + gate.look(idx1, idx2)[0]] += 1
                        turned_away = min(turned_away, dist)
                if best_idx2 >= 0:
                    matches12[idx1] = best_idx2
                    nmatches += 1
                    if turned_away < best_dist:
                        ex["gate_decided"] += 1       # a closer descriptor that the gate turned away lost to a farther one
                    if check_orientation:
                        rot_hist[rot_bin(t1.angle[idx1], t2.angle[best_idx2])].append(idx1)
                else:
                    ex["no_match"] += 1
            i += 1
            j += 1
        elif keys1[i] < keys2[j]:
            ex["node_only_in_1"] += 1
            while i < len(keys1) and keys1[i] < keys2[j]:
                i += 1
        else:
            ex["node_only_in_2"] += 1
            while j < len(keys2) and keys2[j] < keys1[i]:
                j += 1
    if check_orientation:
        keep = three_maxima([len(h) for h in rot_hist])
        for b in range(HISTO_LENGTH):
            if b in keep:
                continue
            for idx1 in rot_hist[b]:
                matches12[idx1] = -1
                nmatches -= 1
                ex["rotation_filtered"] += 1
    return np.array(matches12, np.int32), nmatches


def candidates(t1, t2):
    """(idx1, idx2, dist) of every pair that reaches the gate: one node, no map point on either side, dist <= TH_LOW."""
    fv1, fv2 = feature_vector(t1.node), feature_vector(t2.node)
    out = []
    for node in sorted(set(fv1) & set(fv2)):
        i1 = np.array([i for i in fv1[node] if not t1.has_mp[i]], np.int64)
        i2 = np.array([i for i in fv2[node] if not t2.has_mp[i]], np.int64)
        if len(i1) == 0 or len(i2) == 0:
            continue
        D = POP8[np.bitwise_xor(t1.desc[i1][:, None, :], t2.desc[i2][None, :, :])].sum(-1, dtype=np.int64)
        for a, b in zip(*np.nonzero(D <= TH_LOW)):
            out.append((int(i1[a]), int(i2[b]), int(D[a, b])))
    return out


def search_closed(t1, nb, only_stereo=False, coarse=False, check_orientation=False, gate=None):
    """The closed form: for every idx1 the minimum of (dist << 32) | (0xffffffff - idx2) over the candidates that pass the gate."""
    gate = gate or Gate(t1, nb)
    n1 = len(t1.node)
    best = {}
    if not only_stereo:
        for i1, i2, d in candidates(t1, nb.t2):
            if coarse or gate(i1, i2):
                best[i1] = min(best.get(i1, 1 << 62), (d << 32) | (0xFFFFFFFF - i2))
    matches = np.full(n1, -1, np.int32)
    for i1, k in best.items():
        matches[i1] = 0xFFFFFFFF - (k & 0xFFFFFFFF)
    if check_orientation:
        bins = {int(i): rot_bin(t1.angle[i], nb.t2.angle[matches[i]]) for i in np.nonzero(matches >= 0)[0]}
        keep = three_maxima([list(bins.values()).count(b) for b in range(HISTO_LENGTH)])
        for i, b in bins.items():
            if b not in keep:
                matches[i] = -1
    return matches, int((matches >= 0).sum())


# ---- the constructed corpus -------------------------------------------------------------------------------------------------

POSE_A = pose_from(0.01, -0.02, 0.015, (0.0, 0.0, 0.0))
# B lies 0.33 m behind and beside A (A's centre is in front of B: the epipole is in B's image); C is turned by 80 degrees, 0.45 m
# away: rays that meet in front of a camera of A and BEHIND a camera of C exist (z2), as for RIGS["wide"]
POSE_B = pose_from(0.03, 0.05, -0.02, (0.12, -0.05, -0.30))
POSE_C = pose_from(-0.02, math.radians(-80.0), 0.01, (-0.35, 0.04, 0.28))
COMBOS = ((0, 0), (0, 1), (1, 0), (1, 1))                 # (bRight1, bRight2): ll, lr, rl, rr


def _rig(name, rel, r1, r2):
    """The pair (camera r1 of pKF1, camera r2 of pKF2) as a rig of helpers_geometry, so that fisheye_cases builds its pairs."""
    which = 2 * r1 + r2
    hg.RIGS[name] = (CAMS[r1], CAMS[r2], rel[which, :9].reshape(3, 3).copy(), rel[which, 9:].copy())
    return name


class _Pool:
    """The pairs of one (neighbour, combination), by kind, handed out in order: taking the next one is drawing again."""

    def __init__(self, name, rel, r1, r2, seed, turned):
        rig = _rig(name, rel, r1, r2)
        base = float(np.linalg.norm(rel[2 * r1 + r2, 9:].astype(f64)))
        if turned:
            cases = hg.fisheye_cases(rig, seed, n_ok=30, n_rev=10, n_noise=40, n_z2=16)
        else:
            cases = hg.fisheye_cases(rig, seed, n_ok=60, n_rev=10, n_noise=40, n_corner=8)
            cases += hg.fisheye_cases(rig, seed + 1, n_far=30, depth_scale=base / 0.1)     # straddles cos = 0.9998 for this baseline
        self.by_kind = {}
        for c in cases:
            self.by_kind.setdefault(c["kind"], []).append(c)

    def take(self, kind):
        return self.by_kind[kind].pop(0)


def _project_all(X, rel):
    """A point X (camera 1 of pKF1, left) into the four cameras: ((left, right) of pKF1, (left, right) of pKF2), float64."""
    out1 = [hg.kb8_project64(CAMS[0], X)]
    Tlr = np.eye(4); Tlr[:3, :3] = TLR_R.astype(f64); Tlr[:3, 3] = TLR_T.astype(f64)
    Xr = np.linalg.inv(Tlr) @ np.append(X, 1.0)
    out1.append(hg.kb8_project64(CAMS[1], Xr[:3]))
    out2 = []
    for r2 in (0, 1):
        _, T21 = hg.rig_T21(rel[r2, :9], rel[r2, 9:])                                     # ll, lr: pKF1 left -> pKF2 left / right
        out2.append(hg.kb8_project64(CAMS[r2], T21[:3] @ np.append(X, 1.0)))
    return out1, out2


def build_pair(seed, p1, p2, first_node, turned=False, with_epipole=False, big=False):
    """The features of pKF1 and of one neighbour that belong to each other, as groups: one BoW node and one code row each, so
    that only the pairs of a group reach the gate.  -> (rows1 by side, rows2 by side, refused draws); rows are (x, y, octave, angle,
    desc, node, has_mp) and carry the group's node id."""
    rng = np.random.default_rng(seed)
    rel = relative_poses(p1, p2)
    ep = epipole(p1, p2)
    pools = {c: _Pool("tri2cam_%d_%d%d" % (seed, c[0], c[1]), rel, c[0], c[1], 1000 * seed + 10 * i, turned) for i, c in enumerate(COMBOS)}
    rows1, rows2 = ([], []), ([], [])
    state = {"node": first_node, "redrawn": 0}
    rot0 = rng.uniform(0, 360)

    def angles(aligned=True):
        a1 = rng.uniform(0, 359.9)
        a2 = (a1 - rot0 + rng.normal(0, 3)) % 360 if aligned else rng.uniform(0, 359.9)
        return float(f32(a1)) % 360, (float(f32(a2)) % 360 if float(f32(a2)) < 360 else 0.0)

    def group(make):
        """make() -> (list of (side, x, y, octave, flips, has_mp) for pKF1, the same for pKF2); drawn again while a pair of the
        group that reaches the gate is undecided."""
        while True:
            g1, g2 = make()
            code = hg.code_rows(1, state["node"] % 512)[0]
            a1, a2 = angles(rng.random() < 0.8)
            r1 = [(x, y, o, a1, hg.flip_bits(code, fl, rng) if fl else code.copy(), state["node"], mp, s) for s, x, y, o, fl, mp in g1]
            r2 = [(x, y, o, a2, hg.flip_bits(code, fl, rng) if fl else code.copy(), state["node"], mp, s) for s, x, y, o, fl, mp in g2]
            # the pairs of this group that reach the gate, decided?
            sides1 = [r[7] for r in r1]
            sides2 = [r[7] for r in r2]
            t1 = make_table([r[:7] for r in r1 if r[7] == 0] + [r[:7] for r in r1 if r[7] == 1], sides1.count(0))
            t2 = make_table([r[:7] for r in r2 if r[7] == 0] + [r[:7] for r in r2 if r[7] == 1], sides2.count(0))
            gate = Gate(t1, Neighbour(t2, rel, ep))
            if not any(gate.look(i1, i2)[2] for i1, i2, _ in candidates(t1, t2)):
                break
            state["redrawn"] += 1
        for r in r1:
            rows1[r[7]].append(r[:7])
        for r in r2:
            rows2[r[7]].append(r[:7])
        state["node"] += 1

    def kp(c, which, side, flips=0, mp=0):
        x, y, o = c[which]
        return (side, x, y, o, flips, mp)

    def anywhere(side, flips, octave=None):
        return (side, f32(rng.uniform(60, 450)), f32(rng.uniform(60, 450)), int(rng.integers(0, 8)) if octave is None else octave, flips, 0)

    for (r1, r2), pool in pools.items():
        kinds = (("ok", 8), ("reversed", 4), ("noise", 16), ("behind_cam2", 5)) if turned else \
                (("ok", 8), ("reversed", 3), ("noise", 14), ("corner", 2), ("far", 9))
        for kind, count in kinds:
            for _ in range(count):                    # one pair alone in its node
                group(lambda: (lambda c: ([kp(c, "kp1", r1)], [kp(c, "kp2", r2, int(rng.integers(0, 9)))]))(pool.take(kind)))
        # a closer descriptor at a place the gate turns away, the true feature farther: the gate, not the distance, decides
        for _ in range(2):
            group(lambda: (lambda c: ([kp(c, "kp1", r1)], [anywhere(r2, 2), kp(c, "kp2", r2, 20), anywhere(r2, 0)]))(pool.take("ok")))
        # the true feature three times: equal distances (the last listed wins), then a farther copy (worse than the best)
        group(lambda: (lambda c: ([kp(c, "kp1", r1)], [kp(c, "kp2", r2), kp(c, "kp2", r2), kp(c, "kp2", r2), kp(c, "kp2", r2, 7)]))(
            pool.take("ok")))
        # beyond TH_LOW, and map points on either side
        group(lambda: (lambda c: ([kp(c, "kp1", r1)], [kp(c, "kp2", r2, 51 + int(rng.integers(0, 30)))]))(pool.take("ok")))
        group(lambda: (lambda c: ([kp(c, "kp1", r1, 0, 1)], [kp(c, "kp2", r2)]))(pool.take("ok")))
        group(lambda: (lambda c: ([kp(c, "kp1", r1)], [kp(c, "kp2", r2, 0, 1), kp(c, "kp2", r2, 9)]))(pool.take("ok")))
    # one point seen by all four cameras: features on both sides of NLeft in one node, each pair under its own pose
    for _ in range(2 if turned else 5):
        def quad():
            while True:
                X = hg._direction(rng, 0.05, 0.6) * rng.uniform(0.5, 2.5)
                (l1, rr1), (l2, rr2) = _project_all(X, rel)
                if all(20 < v < 490 for p in (l1, rr1, l2, rr2) for v in p):
                    break
            o = lambda: int(rng.integers(0, 8))
            return ([(0, f32(l1[0]), f32(l1[1]), o(), 0, 0), (1, f32(rr1[0]), f32(rr1[1]), o(), 3, 0)],
                    [(0, f32(l2[0]), f32(l2[1]), o(), 5, 0), (1, f32(rr2[0]), f32(rr2[1]), o(), 5, 0), (1, f32(rr2[0]), f32(rr2[1]), o(), 9, 0)])
        group(quad)
    if with_epipole:
        # accepted pairs whose kp2 lies within 10 sqrt(scale) px of the epipole: :1089-1097 would drop them
        _, T21 = hg.rig_T21(rel[0, :9], rel[0, 9:])
        c1 = T21[:3, 3]                               # pKF1's left centre in pKF2's left camera
        e = c1 / np.linalg.norm(c1)
        for _ in range(3):
            def near_ep():
                a = np.cross(e, rng.normal(size=3)); a /= np.linalg.norm(a)
                X2 = (np.linalg.norm(c1) + rng.uniform(0.6, 0.9)) * (e * math.cos(0.07) + a * math.sin(0.07))
                X1 = hg.rig_T21(rel[0, :9], rel[0, 9:])[0][:3] @ np.append(X2, 1.0)
                p1, p2 = hg.kb8_project64(CAMS[0], X1), hg.kb8_project64(CAMS[0], X2)
                return [(0, f32(p1[0]), f32(p1[1]), int(rng.integers(0, 8)), 0, 0)], [(0, f32(p2[0]), f32(p2[1]), 6, 4, 0)]
            group(near_ep)
    if big:
        # one node with more than 64 candidates: the true features of both cameras many times (ties), decoys between them
        def crowd():
            g1, g2 = quad()
            out2 = []
            for i in range(150):
                out2.append(g2[i % 2][:4] + (0 if i % 3 else 6, 0) if i % 5 else anywhere(i % 2, i % 4))
            return g1, out2
        group(crowd)
    # nodes that one side lists alone, and features in no node
    for side in (0, 1):
        for _ in range(3):
            rows1[side].append((f32(rng.uniform(60, 450)), f32(rng.uniform(60, 450)), 0, 10.0, hg.code_rows(1, 7)[0], state["node"], 0))
            rows2[side].append((f32(rng.uniform(60, 450)), f32(rng.uniform(60, 450)), 0, 10.0, hg.code_rows(1, 7)[0], state["node"] + 1, 0))
            state["node"] += 2
        rows1[side].append((f32(100), f32(100), 0, 10.0, hg.code_rows(1, 9)[0], -1, 0))
        rows2[side].append((f32(100), f32(100), 0, 10.0, hg.code_rows(1, 9)[0], -1, 0))
    return rows1, rows2, rel, ep, state["node"], state["redrawn"]


def _shuffled(rows_by_side, rng):
    """One table: the left camera's rows, then the right camera's, each in a random order."""
    left = [rows_by_side[0][i] for i in rng.permutation(len(rows_by_side[0]))]
    right = [rows_by_side[1][i] for i in rng.permutation(len(rows_by_side[1]))]
    return make_table(left + right, len(left))


_CORPUS = {}


def corpus(big=False):
    """pKF1 = pose A against three neighbours: pose B, pose C, and B's table again with rows dropped and in another order (the
    same groups of pKF1 serve it): (t1, [Neighbour], redrawn)."""
    if big in _CORPUS:
        return _CORPUS[big]
    rng = np.random.default_rng(77)
    rows1, nbrs, node, redrawn = ([], []), [], 0, 0
    for seed, p2, turned, with_ep in ((1, POSE_B, False, True), (2, POSE_C, True, False)):
        r1, r2, rel, ep, node, rd = build_pair(seed, POSE_A, p2, node, turned, with_ep, big and seed == 1)
        rows1[0].extend(r1[0]); rows1[1].extend(r1[1])
        nbrs.append(Neighbour(_shuffled(r2, rng), rel, ep))
        redrawn += rd
        if seed == 1:
            again = tuple([r for r in side if rng.random() > 0.08] for side in r2)
            third = Neighbour(_shuffled(again, rng), rel, ep)
    nbrs.append(third)
    _CORPUS[big] = (_shuffled(rows1, rng), nbrs, redrawn)
    return _CORPUS[big]


SETTINGS = [(co, ori) for co in (False, True) for ori in (False, True)]
EXITS = ("has_mp1", "has_mp2", "th_low", "worse_than_best", "taken", "replaced", "tie_later_wins", "no_match", "rotation_filtered",
         "node_only_in_1", "node_only_in_2", "gate_decided")


def test_scalar_and_closed_form_agree_on_the_corpus_and_every_exit_is_taken():
    t1, nbrs, redrawn = corpus()
    total, labels = Counter(), {c: Counter() for c in COMBOS}
    und = 0
    for nb in nbrs:
        assert 200 <= len(nb.t2.node) <= 400 and 200 <= len(t1.node) <= 400, (len(t1.node), len(nb.t2.node))
        gate = Gate(t1, nb)
        for coarse, ori in SETTINGS:
            ex = Counter()
            m1, n1 = search_scalar(t1, nb, False, coarse, ori, ex, gate)
            m2, n2 = search_closed(t1, nb, False, coarse, ori, gate)
            assert np.array_equal(m1, m2) and n1 == n2 == int((m1 >= 0).sum()), (coarse, ori)
            total.update(ex)
        for i1, i2, _ in candidates(t1, nb.t2):
            lab, mg, u, _ = gate.look(i1, i2)
            und += u
            labels[(int(i1 >= t1.nleft), int(i2 >= nb.t2.nleft))][lab] += 1
    print("corpus: %d + %s features, undecided pairs %d, tables refused 0, keypoints drawn again %d" %
          (len(t1.node), [len(nb.t2.node) for nb in nbrs], und, redrawn))
    print("exits:", dict(total))
    print("labels by (bRight1, bRight2):", {k: dict(v) for k, v in labels.items()})
    assert und == 0
    for name in EXITS:
        assert total[name] > 0, (name, dict(total))
    for c in COMBOS:
        for lab in ("ok", "parallax", "chi1", "chi2"):
            assert labels[c][lab] > 0, (c, lab, dict(labels[c]))
    assert sum(v["z1"] for v in labels.values()) > 0 and sum(v["z2"] for v in labels.values()) > 0


def oracle_pairs(po, pairs, camA, camB, R12, t12):
    """Pairs ((x, y, octave), (x, y, octave)) through pyoracle.stereo_fisheye, as fisheye_table lays tables out: left row i carries
    code row i and so does its partner, every other right row is 128 bits or more away.  -> accepted[n], depth[n], p3d[n, 3]."""
    acc, dep, p3 = [], [], []
    for s in range(0, len(pairs), 256):
        part = pairs[s:s + 256]
        n = len(part)
        codes = hg.code_rows(max(n, 2), 0)
        kl, kr = np.zeros(max(n, 2), hg.KEYPOINT_DT), np.zeros(max(n, 2), hg.KEYPOINT_DT)
        kl["x"], kl["y"], kr["x"], kr["y"] = 250.0, 250.0, 250.0, 250.0
        for i, (a, b) in enumerate(part):
            kl["x"][i], kl["y"][i], kl["octave"][i] = a
            kr["x"][i], kr["y"][i], kr["octave"][i] = b
        _, l2r, _, depth, p3d = po.stereo_fisheye(kl, codes, 0, kr, codes, 0, camA, camB, R12, t12, SIGMA2)
        assert ((l2r[:n] < 0) | (l2r[:n] == np.arange(n))).all()
        acc.extend((l2r[:n] >= 0).tolist()); dep.extend(depth[:n].tolist()); p3.extend(p3d[:n].tolist())
    return np.array(acc, bool), np.array(dep, f64), np.array(p3, f64).reshape(-1, 3)


def measure(po, t1, nb, pairs=None):
    """The deviations of the docstring over the pairs of (t1, nb) that reach the gate: (cos, px, {class: c}, label mismatches)."""
    gate = Gate(t1, nb)
    worst_cos = worst_px = 0.0
    worst_c = {"default": 0.0, "corner": 0.0}
    wrong = 0
    by_combo = {c: [] for c in COMBOS}
    for i1, i2, _ in (pairs if pairs is not None else candidates(t1, nb.t2)):
        by_combo[(int(i1 >= t1.nleft), int(i2 >= nb.t2.nleft))].append((i1, i2))
    for (r1, r2), lst in by_combo.items():
        if not lst:
            continue
        R12, t12 = nb.rel[2 * r1 + r2, :9], nb.rel[2 * r1 + r2, 9:]
        Rd, tn = R12.reshape(3, 3).astype(f64), float(np.linalg.norm(t12.astype(f64)))
        kps = [((t1.x[a], t1.y[a], t1.octave[a]), (nb.t2.x[b], nb.t2.y[b], nb.t2.octave[b])) for a, b in lst]
        acc, depth, p3d = oracle_pairs(po, kps, CAMS[r1], CAMS[r2], R12, t12)
        for n, (a, b) in enumerate(lst):
            lab, mg, _, corner = gate.look(a, b)
            wrong += int(acc[n] != (lab == "ok"))
            if "_cos" in mg:
                q1 = po.kb8_unproject(CAMS[r1], t1.x[a], t1.y[a]).astype(f64)
                q2 = Rd @ po.kb8_unproject(CAMS[r2], nb.t2.x[b], nb.t2.y[b]).astype(f64)
                worst_cos = max(worst_cos, abs(q1 @ q2 / (np.linalg.norm(q1) * np.linalg.norm(q2)) - mg["_cos"]) + 2.0 ** -24)
            if lab == "ok" and acc[n]:
                _, _, X = hg.fisheye_expect(kps[n][0], kps[n][1], CAMS[r1], CAMS[r2], R12, t12, SIGMA2)
                unit = hg.EPS32 * max(1.0, X[2] * X[2] / tn)
                c = max(abs(depth[n] - X[2]), float(np.abs(p3d[n] - X).max())) / unit
                worst_c["corner" if corner else "default"] = max(worst_c["corner" if corner else "default"], c)
                uv = po.kb8_project(CAMS[r1], p3d[n].astype(f32)).astype(f64)
                e1 = math.hypot(uv[0] - float(t1.x[a]), uv[1] - float(t1.y[a]))
                worst_px = max(worst_px, abs(e1 - mg["_e1"]))
    return worst_cos, worst_px, worst_c, wrong


def test_margins_are_measured_against_the_oracle_and_labels_agree(oracle):
    worst_cos = worst_px = 0.0
    worst_c = {"default": 0.0, "corner": 0.0}
    npairs = 0
    for big in (False, True):
        t1, nbrs, _ = corpus(big)
        for nb in nbrs:
            co, px, c, wrong = measure(oracle, t1, nb)
            npairs += len(candidates(t1, nb.t2))
            assert wrong == 0
            worst_cos, worst_px = max(worst_cos, co), max(worst_px, px)
            worst_c = {k: max(worst_c[k], c[k]) for k in c}
    print("two-camera triangulation, %d pairs: oracle vs float64 cos %.3g (recorded %.3g), reprojection %.3g px (recorded %.3g), c %s "
          "(recorded %s); decided margins %s" % (npairs, worst_cos, MEASURED_COS, worst_px, MEASURED_REPROJ_PX, worst_c, MEASURED_C, MARGIN))
    assert worst_cos <= MEASURED_COS and worst_px <= MEASURED_REPROJ_PX and all(worst_c[k] <= MEASURED_C[k] for k in worst_c), \
        "the recorded worst deviations are out of date"


# ---- hand-worked known answers ---------------------------------------------------------------------------------------------

Z = np.zeros(32, np.uint8)


def _one_point():
    """One point in front of A and B and its four images, as float32 keypoints at octave 2."""
    rel = relative_poses(POSE_A, POSE_B)
    (l1, r1), (l2, r2) = _project_all(np.array([0.2, -0.1, 1.5]), rel)
    k = lambda p: (f32(p[0]), f32(p[1]), 2, 0.0)
    return rel, k(l1), k(r1), k(l2), k(r2)


def run(rows1, nleft1, rows2, nleft2, rel, **kw):
    t1, nb = make_table(rows1, nleft1), Neighbour(make_table(rows2, nleft2), rel, (1e6, 1e6))
    m, n = search_scalar(t1, nb, **kw)
    m2, n2 = search_closed(t1, nb, **kw)
    assert np.array_equal(m, m2) and n == n2
    return m.tolist(), n


def test_only_stereo_returns_nothing_and_coarse_takes_the_closest():
    rel, l1, r1, l2, r2 = _one_point()
    away = (f32(400.0), f32(90.0), 2, 0.0)            # nowhere near the point's image: the gate turns it away
    kf1 = [l1 + (Z, 4)]
    kf2 = [away + (Z, 4), l2 + (desc_with_bits(10), 4)]
    assert run(kf1, 1, kf2, 2, rel) == ([1], 1)                         # the farther descriptor, the only one the gate lets through
    assert run(kf1, 1, kf2, 2, rel, coarse=True) == ([0], 1)            # bCoarse: the closest, whatever the gate says
    assert run(kf1, 1, kf2, 2, rel, only_stereo=True) == ([-1], 0)      # bStereo1 is false for every feature
    assert run(kf1, 1, [away + (Z, 4)], 1, rel) == ([-1], 0)
    assert run(kf1, 1, [l2 + (desc_with_bits(51), 4)], 1, rel, coarse=True) == ([-1], 0)        # TH_LOW holds under bCoarse


def test_indices_run_over_n_and_the_side_picks_the_pose():
    rel, l1, r1, l2, r2 = _one_point()
    # pKF1: one left feature (in no node) and the right image of the point; pKF2: two left features, the second the point's
    kf1 = [(f32(50), f32(50), 0, 0.0, Z, -1), r1 + (Z, 4)]
    kf2 = [(f32(300), f32(300), 0, 0.0, desc_with_bits(60), 4), l2 + (Z, 4), r2 + (desc_with_bits(3), 4)]
    assert run(kf1, 1, kf2, 2, rel) == ([-1, 1], 1)                     # idx1 = 1 >= NLeft: pose rl, then rr for idx2 = 2
    # only the right feature of pKF2 left: pose rr
    assert run(kf1, 1, kf2[::2], 1, rel) == ([-1, 1], 1)
    # of equal distances the last listed wins, across NLeft
    kf2 = [l2 + (Z, 4), r2 + (Z, 4)]
    assert run([l1 + (Z, 4)], 1, kf2, 1, rel) == ([1], 1)
    assert run([l1 + (Z, 4)], 1, [kf2[0], kf2[0]], 2, rel) == ([1], 1)


def test_relative_poses_are_the_poses_of_the_rig():
    """The float32 gemm chain against float64 homogeneous matrices; the right camera sits 0.1 m from the left one."""
    Tlr = np.eye(4); Tlr[:3, :3] = TLR_R; Tlr[:3, 3] = TLR_T
    T = lambda p, right: (np.linalg.inv(Tlr) if right else np.eye(4)) @ np.vstack([np.hstack([p.R.astype(f64), p.t.astype(f64)]), [0, 0, 0, 1]])
    rel = relative_poses(POSE_A, POSE_C)
    for r1, r2 in COMBOS:
        want = T(POSE_A, r1) @ np.linalg.inv(T(POSE_C, r2))
        got = rel[2 * r1 + r2]
        assert np.abs(got[:9].reshape(3, 3) - want[:3, :3]).max() < 1e-6 and np.abs(got[9:] - want[:3, 3]).max() < 1e-6
    assert not np.array_equal(rel[1], rel[2])


# ---- mutations ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("switch", ["rl_for_lr", "wrong_camera", "swap_sigmas", "first_wins", "epipole_gate"])
def test_the_corpus_tells_a_wrong_reading_apart(switch):
    t1, nbrs, _ = corpus()
    rules = replace(REF, **{switch: True})
    caught = 0
    for nb in nbrs:
        want = search_closed(t1, nb)[0]
        got = search_scalar(t1, nb, gate=Gate(t1, nb, rules))[0]
        caught += int((want != got).sum())
    print("mutation %s: %d rows differ" % (switch, caught))
    assert caught > 0


# ---- extracted tables ---------------------------------------------------------------------------------------------------------

SCENE_W = SCENE_H = 512
SCENE_SHIFTS = ((0, 44), (0, 20), (1, 44), (1, 0))       # (frame, window offset) of pKF1 and of the three neighbours


def scene_config():
    from pli_slam_amd import capi
    return capi.default_config(SCENE_W, SCENE_H, orb_nfeatures=300, lsd_nfeatures=20, max_frames=1)


def scene_images(seed=3):
    from pli_slam_amd import synth
    out = []
    for t, shift in SCENE_SHIFTS:
        L, R = synth.make_stereo_pair(seed, 560, SCENE_H, t=t)
        out.append((np.ascontiguousarray(L[:, shift:shift + SCENE_W]), np.ascontiguousarray(R[:, shift:shift + SCENE_W])))
    return out


def scene_poses():
    """pKF1 and three neighbours beside it: the window offsets and the frame step read as sideways motion of a rig looking at a
    wall about 2.5 m away.  Any fixed poses serve: the test is parity with the restatement."""
    p1 = pose_from(0.0, 0.0, 0.0, (0.0, 0.0, 0.0))
    return p1, [pose_from(0.0, 0.0, 0.0, (-0.30, 0.0, 0.0)), pose_from(0.002, -0.003, 0.0087, (0.04, 0.013, 0.0)),
                pose_from(0.002, -0.003, 0.0087, (-0.55, -0.013, 0.01))]


def scene_tables(extract, nodes_of, seed=3):
    """extract(image) -> (kp, desc) and nodes_of(desc) -> node per feature, by the device or by the oracle.  -> (t1, [Neighbour])."""
    rng = np.random.default_rng(seed)
    tables = []
    for L, R in scene_images(seed):
        (kl, dl), (kr, dr) = extract(L), extract(R)
        kp, desc = np.concatenate([kl, kr]), np.concatenate([dl, dr])
        assert kp["angle"].min() >= 0 and kp["angle"].max() < 360
        tables.append(Table(kp["x"].astype(f32), kp["y"].astype(f32), kp["octave"].astype(np.int32), kp["angle"].astype(f32), desc.copy(),
                            nodes_of(desc).astype(np.int32), (rng.random(len(kp)) < 0.2).astype(np.uint8), len(kl)))
    p1, p2s = scene_poses()
    return tables[0], [Neighbour(t, relative_poses(p1, p), epipole(p1, p)) for t, p in zip(tables[1:], p2s)]


def scene_rows(t1, nb):
    """-> (gate, rows of pKF1 that have a candidate within TH_LOW, those of them that have an undecided candidate)."""
    gate = Gate(t1, nb)
    have, und = set(), set()
    for i1, i2, _ in candidates(t1, nb.t2):
        have.add(i1)
        if gate.look(i1, i2)[2]:
            und.add(i1)
    return gate, have, und


def test_the_extracted_scene_leaves_out_at_most_two_percent_of_its_rows(oracle):
    """The cap the GPU test puts on rows with an undecided candidate, here on the same scene with the float64 statement alone (the
    oracle's extractor and vocabulary give the tables the device gives); every neighbour keeps matches."""
    from pli_slam_amd import synth
    cfg = oracle.Config.from_buffer_copy(bytes(scene_config()))
    fr = oracle.Frame(cfg)
    voc = oracle.Vocabulary(*synth.make_vocabulary(10, 4, seed=0))

    def extract(img):
        n, kp, desc = fr.orb_extract(0, img)
        return kp[:n].copy(), desc[:n].copy()

    def nodes_of(desc):
        _, weight, node = voc.descend(desc, 2)
        return np.where(weight > 0, node, -1)
    t1, nbrs = scene_tables(extract, nodes_of)
    for k, nb in enumerate(nbrs):
        gate, have, und = scene_rows(t1, nb)
        m, n = search_closed(t1, nb, gate=gate)
        print("scene neighbour %d: %d + %d features, %d rows with a candidate, %d left out (%.2f %%), %d matches" %
              (k, len(t1.node), len(nb.t2.node), len(have), len(und), 100.0 * len(und) / max(len(have), 1), n))
        assert len(have) > 50 and len(und) <= 0.02 * len(have) and n > 0


# ---- the adapter ---------------------------------------------------------------------------------------------------------------

def test_two_camera_triangulation_harness_builds_and_fails_loudly_without_a_device(tmp_path):
    """Here (no GPU) the first library call throws pli::Error(PLI_ERR_NO_DEVICE) and the harness exits with 1; on the GPU box the
    same program runs.  Either way PliORBmatcherTwoCameras::SearchForTriangulation compiles against the stub types and links."""
    import torch
    from test_cpp_triangulation_two_cameras import build, write_input
    exe = build(str(tmp_path))
    t1, nbrs, _ = corpus()
    inp, outp = str(tmp_path / "in"), str(tmp_path / "out")
    write_input(inp, t1, nbrs[:1], [POSE_B], False, True)
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300)
    if torch.cuda.is_available():
        assert r.returncode == 0, r.stderr
    else:
        assert r.returncode == 1 and "no HIP device" in r.stderr, (r.returncode, r.stderr)


def test_the_header_declares_the_entry_point():
    src = open(os.path.join(ROOT, "include", "pli_frontend.h")).read()
    assert "pli_status pli_search_for_triangulation_two_cameras(" in src
    from pli_slam_amd import capi
    assert "pli_search_for_triangulation_two_cameras" in capi._PROTOS
