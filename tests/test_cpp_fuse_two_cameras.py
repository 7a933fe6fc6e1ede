"""The C++ Fuse adapters for keyframes of two cameras, executed (-m gpu): tests/cpp/fuse_two_cameras_harness.cpp runs
PliORBmatcherTwoCameras::Fuse(pKF, vpMapPoints, th) and Fuse(pKF, vpMapPoints, th, true) keyframe after keyframe, in the order of
LocalMapping.cc:747-748, and the batch form once, on two copies of the same stub state whose MapPoint::Replace moves observations
and installs another descriptor on the survivor.  Both dumps (return values per keyframe and side, every keyframe's mvpMapPoints, the
bad flags) equal a Python simulation of ORBmatcher.cc:1572-1594 over the restatement of tests/test_fuse_two_cameras_cpu.py,
searched view by view with the descriptors as they are at that time; the batch form must have repeated a search at least once, and
at least one point must have been added on the left of a keyframe and skipped on its right (:1448).  Also: a keyframe of one camera
is forwarded to the base, and the two refusals (a mixed target list, mvuRight >= 0).  The level_ratio table is the one the adapter
built with this host's compiler (dumped)."""
import os
import subprocess

import numpy as np
import pytest

from test_fuse_search_cpu import NLEVELS
from test_fuse_two_cameras_cpu import BOUNDS, CAMS, fuse2_case, fuse2_fast
from test_triangulation_two_cameras_cpu import TLR_R, TLR_T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "pli_slam_amd", "csrc", "libpli_frontend.so")


def build(outdir):
    exe = os.path.join(outdir, "fuse_two_cameras_harness")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", "-pthread", "-I", ROOT, "-I",
                        os.path.join(ROOT, "tests", "stubs"), os.path.join(ROOT, "tests", "cpp", "fuse_two_cameras_harness.cpp"),
                        LIB, "-Wl,-rpath," + os.path.dirname(LIB), "-Wl,-rpath,/opt/rocm/lib", "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def make_world(seed, nkf, npool, nfeat=(160, 120)):
    """A pool of points; the list = most of the pool, some twice, some null; every keyframe feature holds a pool point with
    probability 0.5 (so that most matches meet a map point and Replace runs), with random observation counts."""
    C = fuse2_case(seed, nkf, npool, nfeat)
    rng = np.random.default_rng(seed + 1000)
    pts, descs = C.pts, C.descs
    alt = rng.integers(0, 256, (npool, 32), dtype=np.uint8)
    # half of the alternative descriptors stay close to the first one, so that the repeated search still finds matches
    near = rng.random(npool) < 0.5
    alt[near] = descs[near] ^ np.left_shift(1, rng.integers(0, 8, (int(near.sum()), 32))).astype(np.uint8) * (rng.random((int(near.sum()), 32)) < 0.2)
    obs0 = rng.integers(0, 6, npool).astype(np.int32)
    lst = np.concatenate([rng.permutation(npool)[:int(npool * 0.8)], rng.integers(0, npool, 20), [-1, -1]]).astype(np.int32)
    lst = rng.permutation(lst)
    held = []
    for kf in C.kfs:
        mp = np.where(rng.random(len(kf.x)) < 0.5, rng.integers(0, npool, len(kf.x)), -1).astype(np.int32)
        _, first = np.unique(mp, return_index=True)             # a point is observed at most once per keyframe
        keep = np.zeros(len(mp), bool); keep[first] = True
        mp[~keep] = -1
        held.append(mp)
    return pts, descs, alt, obs0, lst, C.kfs, held


def write_input(path, world, th):
    pts, descs, alt, obs0, lst, kfs, held = world
    tlr = np.concatenate([TLR_R, TLR_T.reshape(3, 1)], 1).astype(np.float32)
    with open(path, "wb") as f:
        f.write(np.array([len(kfs), len(pts), len(lst)], np.int32).tobytes())
        f.write(np.array(list(CAMS[0]) + list(CAMS[1]), np.float32).tobytes() + tlr.tobytes())
        f.write(np.array([BOUNDS.min_x, BOUNDS.max_x, BOUNDS.min_y, BOUNDS.max_y, th], np.float32).tobytes())
        f.write(lst.tobytes() + pts.tobytes() + np.ascontiguousarray(descs).tobytes() + np.ascontiguousarray(alt).tobytes() + obs0.tobytes())
        for kf, mp in zip(kfs, held):
            f.write(np.array([len(kf.x), kf.nleft], np.int32).tobytes() + kf.pose[0, :12].astype(np.float32).tobytes() +
                    kf.x.tobytes() + kf.y.tobytes() + kf.octave.tobytes() + np.ascontiguousarray(kf.desc).tobytes() + mp.tobytes())


def simulate(world, th, lr):
    """The reference's loop: Fuse(KF_k), Fuse(KF_k, ..., bRight = true) for k in order, every search with the state of that
    moment.  -> nFused[2 nkf], mvpMapPoints per keyframe, bad flags, points added on the left and skipped on the right."""
    pts, descs, alt, obs0, lst, kfs, held = world
    npool = len(pts)
    desc = descs.copy()
    bad = pts["valid"] == 0
    obs0 = obs0.copy()
    kfmp = [mp.copy() for mp in held]
    obs = [dict() for _ in range(npool)]              # point -> {keyframe: feature}
    for k, mp in enumerate(kfmp):
        for i, p in enumerate(mp):
            if p >= 0:
                obs[p].setdefault(k, i)

    def replace(a, b):                                # a->Replace(b), MapPoint.cc:232-276
        if a == b:
            return
        o, obs[a] = obs[a], dict()
        bad[a] = True
        for kk in sorted(o):
            if kk not in obs[b]:
                kfmp[kk][o[kk]] = b
                obs[b][kk] = o[kk]
            else:
                kfmp[kk][o[kk]] = -1
        obs0[b] += obs0[a]
        desc[b] = alt[b]
    nfused, skipped_on_right = [], 0
    for k, kf in enumerate(kfs):
        added_left = set()
        for right in (False, True):
            cur = pts.copy()
            cur["valid"] = (~bad).astype(np.int32)
            best, _ = fuse2_fast(cur, desc, kf, right, th, None, lr)
            n = 0
            for p in lst:
                if p < 0 or bad[p]:
                    continue
                if k in obs[p]:
                    skipped_on_right += right and p in added_left and best[p] >= 0
                    continue
                j = int(best[p])
                if j < 0:
                    continue
                q = int(kfmp[k][j])
                if q >= 0:
                    if not bad[q]:
                        if obs0[q] + len(obs[q]) > obs0[p] + len(obs[p]):
                            replace(p, q)
                        else:
                            replace(q, p)
                else:
                    obs[p].setdefault(k, j)
                    kfmp[k][j] = p
                    if not right:
                        added_left.add(int(p))
                n += 1
            nfused.append(n)
    return np.array(nfused, np.int32), kfmp, bad.astype(np.int32), skipped_on_right


@pytest.mark.gpu
def test_two_camera_fuse_adapters_equal_the_reference_loop(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    exe = build(str(tmp_path))
    researched = skipped = 0
    for seed, nkf, npool, th in ((141, 4, 300, 3.0), (142, 2, 250, 4.0)):
        world = make_world(seed, nkf, npool)
        inp, outp = str(tmp_path / "in"), str(tmp_path / "out")
        write_input(inp, world, th)
        r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        raw = np.fromfile(outp, np.int32)
        nfeat = [len(kf.x) for kf in world[5]]
        block = 2 * nkf + sum(nfeat) + npool + 1
        lr = raw[2 * block:2 * block + NLEVELS - 1].view(np.float32)
        assert (np.diff(lr) > 0).all() and abs(lr[1] - 1.2) < 1e-5
        want_n, want_mp, want_bad, on_right = simulate(world, th, lr)
        skipped += on_right
        assert want_n[0::2].sum() > 10 and want_n[1::2].sum() > 10, want_n
        assert want_bad.sum() > (world[0]["valid"] == 0).sum(), "the case replaces nothing"
        for call in range(2):                         # the single calls, then the batch call
            got = raw[call * block:(call + 1) * block]
            assert np.array_equal(got[:2 * nkf], want_n), (call, got[:2 * nkf], want_n)
            at = 2 * nkf
            for k in range(nkf):
                assert np.array_equal(got[at:at + nfeat[k]], want_mp[k]), (call, k)
                at += nfeat[k]
            assert np.array_equal(got[at:at + npool], want_bad), call
        assert raw[block - 1] == 0
        researched += int(raw[2 * block - 1])
        tail = raw[2 * block + NLEVELS - 1:]
        assert tail[0] == tail[1] and tail[0] >= 0, tail       # the one-camera keyframe: this class and the base agree
        assert tail[2:].tolist() == [1, 1], tail               # the mixed list and mvuRight >= 0 are refused
    assert researched >= 1, "the batch form never had to search again: the test does not reach that path"
    assert skipped >= 1, "no point was added on the left of a keyframe and skipped on its right"


def test_two_camera_fuse_harness_builds_and_fails_loudly_without_a_device(tmp_path):
    """Here (no GPU) the extractor call throws pli::Error(PLI_ERR_NO_DEVICE) and the harness exits with 1; on the GPU box the
    same program runs.  Either way it builds and links against the product library."""
    import torch
    exe = build(str(tmp_path))
    world = make_world(5, 2, 60, (30, 20))
    inp, outp = str(tmp_path / "in"), str(tmp_path / "out")
    write_input(inp, world, 3.0)
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300)
    if torch.cuda.is_available():
        assert r.returncode == 0, r.stderr
    else:
        assert r.returncode == 1 and "no HIP device" in r.stderr, (r.returncode, r.stderr)
