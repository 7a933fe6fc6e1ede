"""The C++ SearchByProjection(KeyFrame, Scw, ...) adapters, executed (-m gpu): tests/cpp/sim3_projection_harness.cpp runs the two
reference signatures of PliORBmatcher::SearchByProjection (ORBmatcher.cc:473-586 and :588-704) keyframe by keyframe and the batch
form once, on stub KeyFrame / MapPoint types: vpMatched partly filled at entry (occupied rows, and points already found), bad
points in the list, points listed twice, vpMatchedKF written.  The containers equal the restatement of
tests/test_sim3_projection_cpu.py: project_form 0 for the form without vpPointsKFs and for the batch form, 1 for the other.  The
level_ratio table and the poses are the ones the adapter built with this host's compiler (dumped), since its log(float) and the
Sim3 decomposition need not be Python's to the last bit."""
import os
import subprocess

import numpy as np
import pytest

from test_fuse_search_cpu import CAM, NLEVELS
from test_sim3_projection_cpu import sim3_case, sim3_search_fast

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "pli_slam_amd", "csrc", "libpli_frontend.so")


def build(outdir):
    exe = os.path.join(outdir, "sim3_projection_harness")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", "-pthread", "-I", ROOT, "-I",
                        os.path.join(ROOT, "tests", "stubs"), os.path.join(ROOT, "tests", "cpp", "sim3_projection_harness.cpp"),
                        LIB, "-Wl,-rpath," + os.path.dirname(LIB), "-Wl,-rpath,/opt/rocm/lib", "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def make_world(rng, nkf, npool, nfeat=300, scale=1.3):
    """A pool of points (some bad); the list = the pool shuffled, a quarter of it twice; a tenth of every keyframe's rows hold a
    pool point at entry; Scw = scale * [Rcw | tcw]."""
    pts, descs, kfs, _, _ = sim3_case(rng, nkf, npool, nfeat)
    lst = rng.permutation(np.concatenate([np.arange(npool), rng.integers(0, npool, npool // 4)])).astype(np.int32)
    lst_kf = rng.integers(0, nkf, len(lst)).astype(np.int32)
    held, scw = [], []
    for kf in kfs:
        mp = np.where(rng.random(len(kf.x)) < 0.1, rng.integers(0, npool, len(kf.x)), -1).astype(np.int32)
        held.append(mp)
        S = np.eye(4, dtype=np.float32)
        S[:3, :3] = np.float32(scale) * kf.pose[:9].reshape(3, 3)
        S[:3, 3] = np.float32(scale) * kf.pose[9:12]
        scw.append(S)
    return pts, descs, lst, lst_kf, kfs, held, scw


def write_input(path, world, th, ratio):
    pts, descs, lst, lst_kf, kfs, held, scw = world
    with open(path, "wb") as f:
        f.write(np.array([len(kfs), len(pts), len(lst)], np.int32).tobytes())
        f.write(np.array(list(CAM) + [th, ratio], np.float32).tobytes())
        f.write(lst.tobytes() + lst_kf.tobytes() + pts.tobytes() + np.ascontiguousarray(descs).tobytes())
        for kf, mp, S in zip(kfs, held, scw):
            f.write(np.int32(len(kf.x)).tobytes() + S.astype(np.float32).tobytes() + kf.x.tobytes() + kf.y.tobytes() +
                    kf.octave.tobytes() + np.ascontiguousarray(kf.desc).tobytes() + mp.tobytes())


def expected(world, k, pose, th, ratio, form, lr):
    """-> nmatches, vpMatched (pool indices), vpMatchedKF (keyframe indices) of keyframe k"""
    pts, descs, lst, lst_kf, kfs, held, _ = world
    entry = held[k]
    found = set(entry[entry >= 0].tolist())
    skip = np.array([p in found for p in lst.tolist()], np.uint8)
    rows, _, n = sim3_search_fast(pts[lst], descs[lst], kfs[k]._replace(pose=pose), CAM, th, ratio, form, skip, entry >= 0, lr)
    took = rows >= 0
    matched, matched_kf = entry.copy(), np.full(len(entry), -1, np.int32)
    matched[took] = lst[rows[took]]
    matched_kf[took] = lst_kf[rows[took]]
    return n, matched, matched_kf


@pytest.mark.gpu
def test_the_three_adapter_forms_equal_the_restatement(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    exe = build(str(tmp_path))
    for seed, nkf, npool, th, ratio in ((51, 3, 300, 8, 1.5), (52, 5, 200, 3, 1.5), (53, 1, 250, 5, 1.0)):
        world = make_world(np.random.default_rng(seed), nkf, npool)
        inp, outp = str(tmp_path / "in"), str(tmp_path / "out")
        write_input(inp, world, th, ratio)
        r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        raw = np.fromfile(outp, np.int32)
        nfeat = [len(kf.x) for kf in world[4]]
        tail = raw[sum(2 + 3 * n for n in nfeat) + sum(1 + n for n in nfeat):].view(np.float32)
        lr, poses = tail[:NLEVELS - 1], tail[NLEVELS - 1:].reshape(nkf, 15)
        assert (np.diff(lr) > 0).all() and abs(lr[1] - 1.2) < 1e-5
        at, total = 0, 0
        for k in range(nkf):
            assert np.abs(poses[k][:12] - world[4][k].pose[:12]).max() < 1e-5      # scale * [R | t] decomposes to [R | t]
            n = nfeat[k]
            want4 = expected(world, k, poses[k], th, ratio, 0, lr)
            assert raw[at] == want4[0] and np.array_equal(raw[at + 1:at + 1 + n], want4[1]), ("no vpPointsKFs", k)
            at += 1 + n
            want6 = expected(world, k, poses[k], th, ratio, 1, lr)
            assert raw[at] == want6[0] and np.array_equal(raw[at + 1:at + 1 + n], want6[1]), ("vpPointsKFs", k)
            assert np.array_equal(raw[at + 1 + n:at + 1 + 2 * n], want6[2]), ("vpMatchedKF", k)
            at += 1 + 2 * n
            total += want4[0] + want6[0]
            assert (want4[1] != world[5][k]).sum() == want4[0]
        for k in range(nkf):                          # the batch form
            n = nfeat[k]
            want = expected(world, k, poses[k], th, ratio, 0, lr)
            assert raw[at] == want[0] and np.array_equal(raw[at + 1:at + 1 + n], want[1]), ("batch", k)
            at += 1 + n
        assert total > 40 * nkf, "the case matches nothing"


def test_sim3_projection_harness_builds_and_fails_loudly_without_a_device(tmp_path):
    """Here (no GPU) the extractor call throws pli::Error(PLI_ERR_NO_DEVICE) and the harness exits with 1; on the GPU box the
    same program runs.  Either way it builds and links against the product library."""
    import torch
    exe = build(str(tmp_path))
    world = make_world(np.random.default_rng(1), 2, 60, 50)
    inp, outp = str(tmp_path / "in"), str(tmp_path / "out")
    write_input(inp, world, 3, 1.5)
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300)
    if torch.cuda.is_available():
        assert r.returncode == 0, r.stderr
    else:
        assert r.returncode == 1 and "no HIP device" in r.stderr, (r.returncode, r.stderr)
