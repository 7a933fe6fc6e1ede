"""The C++ SearchForTriangulation adapters for keyframes of two cameras, executed (-m gpu):
tests/cpp/triangulation_two_cameras_harness.cpp calls PliORBmatcherTwoCameras::SearchForTriangulation(pKF1, pKF2, F12,
vMatchedPairs, bOnlyStereo, bCoarse) per neighbour and the batch form once, on stub KeyFrame types that carry mvKeys / mvKeysRight,
NLeft, mTlr and the right-pose getters of KeyFrame.cc:1343-1373.  The dumped pair lists and return values equal the Python
restatement of tests/test_triangulation_two_cameras_cpu.py, whose relative poses restate the stub cv::Mat's arithmetic (one gemm
per product), so the host arithmetic needs no tolerance.  A pair of keyframes without second cameras goes through the same class
and equals the one-camera restatement (tests/test_triangulation_search_cpu.py); a call that mixes the two kinds, and one whose
keyframes differ in their camera parameters, throw std::logic_error."""
import os
import subprocess

import numpy as np
import pytest

import test_triangulation_search_cpu as one
import test_triangulation_two_cameras_cpu as two

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "pli_slam_amd", "csrc", "libpli_frontend.so")
f32 = np.float32


def build(outdir):
    exe = os.path.join(outdir, "triangulation_two_cameras_harness")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", "-pthread", "-I", ROOT, "-I",
                        os.path.join(ROOT, "tests", "stubs"), os.path.join(ROOT, "tests", "cpp", "triangulation_two_cameras_harness.cpp"),
                        LIB, "-Wl,-rpath," + os.path.dirname(LIB), "-Wl,-rpath,/opt/rocm/lib", "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def table_bytes(t, pose, nleft, two_cameras):
    return (np.array([len(t.node), nleft, int(two_cameras)], np.int32).tobytes() + pose.R.astype(f32).tobytes() +
            pose.t.astype(f32).tobytes() + t.x.tobytes() + t.y.tobytes() + t.octave.tobytes() + t.angle.tobytes() +
            np.ascontiguousarray(t.desc).tobytes() + t.node.tobytes() + t.has_mp.tobytes())


def write_input(path, t1, nbrs, poses2, only_stereo, coarse, ori=True, pose1=two.POSE_A, two_cameras=True):
    """nbrs: Neighbour (or any tuple whose first entry is the table) per neighbour, poses2 their poses."""
    with open(path, "wb") as f:
        f.write(np.array([len(nbrs), int(only_stereo), int(coarse), int(ori)], np.int32).tobytes())
        f.write(np.asarray(two.CAMS[0], f32).tobytes() + np.asarray(two.CAMS[1], f32).tobytes())
        f.write(np.hstack([two.TLR_R, two.TLR_T.reshape(3, 1)]).astype(f32).tobytes())
        f.write(table_bytes(t1, pose1, getattr(t1, "nleft", -1), two_cameras))
        for nb, p in zip(nbrs, poses2):
            f.write(table_bytes(nb[0], p, getattr(nb[0], "nleft", -1), two_cameras))


def run(exe, tmp_path, *args, **kw):
    inp, outp = str(tmp_path / "in"), str(tmp_path / "out")
    write_input(inp, *args, **kw)
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return np.fromfile(outp, np.int32)


@pytest.mark.gpu
def test_two_camera_adapters_equal_the_restatement(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    exe = build(str(tmp_path))
    t1, nbrs, _ = two.corpus()
    poses2 = [two.POSE_B, two.POSE_C, two.POSE_B]
    n1 = len(t1.node)
    for only_stereo, coarse, ori in ((False, False, True), (False, False, False), (False, True, True), (True, False, True)):
        raw = run(exe, tmp_path, t1, nbrs, poses2, only_stereo, coarse, ori)
        nkf = len(nbrs)
        got = raw[:2 * nkf * (n1 + 1)].reshape(2, nkf, n1 + 1)
        assert raw[2 * nkf * (n1 + 1):].tolist() == [1, 1], "the two refusals"
        total = 0
        for k, nb in enumerate(nbrs):
            want_m, want_n = two.search_closed(t1, nb, only_stereo, coarse, ori)
            for call in range(2):                   # single calls, then the batch call
                assert got[call, k, 0] == want_n, (call, k, got[call, k, 0], want_n)
                assert np.array_equal(got[call, k, 1:], want_m), (call, k, int((got[call, k, 1:] != want_m).sum()))
            total += want_n
        assert (total > 0) != only_stereo


@pytest.mark.gpu
def test_keyframes_of_one_camera_are_forwarded(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    exe = build(str(tmp_path))
    poses = []
    t1, nbrs = one.two_view_case(np.random.default_rng(41), 2, 300, 20, poses=poses)
    mono = lambda t: t._replace(stereo=np.zeros_like(t.stereo))          # (the harness sets no mvuRight)
    t1 = mono(t1)
    nbrs = [(mono(nb[0]),) + tuple(nb[1:]) for nb in nbrs]
    as_pose = lambda R, t: two.Pose(np.asarray(R, f32), np.asarray(t, f32))
    raw = run(exe, tmp_path, t1, nbrs, [as_pose(p[2], p[3]) for p in poses], False, False, True,
              pose1=as_pose(poses[0][0], poses[0][1]), two_cameras=False)
    n1, nkf = len(t1.node), len(nbrs)
    got = raw[:2 * nkf * (n1 + 1)].reshape(2, nkf, n1 + 1)
    geo = raw[2 * nkf * (n1 + 1):].view(np.float32).reshape(nkf, 11)
    total = 0
    for k, nb in enumerate(nbrs):
        want_m, want_n = one.search_for_triangulation_fast(t1, nb[0], geo[k, :9].reshape(3, 3), geo[k, 9:], False, False, True)
        for call in range(2):
            assert got[call, k, 0] == want_n and np.array_equal(got[call, k, 1:], want_m), (call, k)
        total += want_n
    assert total > 0
