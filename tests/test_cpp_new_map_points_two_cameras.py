"""The C++ adapter PliCreateNewMapPointsTwoCameras (pli_slam_amd/adapters/orbslam_local_mapping_two_cameras.hpp), executed
(-m gpu): tests/cpp/new_map_points_two_cameras_harness.cpp runs it on stub KeyFrame / MapPoint / Atlas types that log every call
of LocalMapping.cc:670-683.  The dumped order of the calls, mlpRecentAddedMapPoints and the positions equal what the Python
restatement of the reference's loop (tests/helpers_new_map_points_two_cameras.py) creates, also with a CheckNewKeyFrames() that
answers true before neighbour 2; the harness's own sequence "one SearchForTriangulation per neighbour, then the replay of what the
adapter created there" on a copy of the state equals the loop's searches; a mixed call and cameras that differ throw; a call of
one-camera keyframes is forwarded and equals the one-camera restatement (tests/helpers_new_map_points.py)."""
import os
import subprocess

import numpy as np
import pytest

import helpers_new_map_points as H1
import helpers_new_map_points_two_cameras as h
import test_triangulation_two_cameras_cpu as two
from test_cpp_new_map_points import expected_log

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "pli_slam_amd", "csrc", "libpli_frontend.so")
f32 = np.float32


def build(outdir):
    exe = os.path.join(outdir, "new_map_points_two_cameras_harness")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", "-pthread", "-I", ROOT, "-I",
                        os.path.join(ROOT, "tests", "stubs"), os.path.join(ROOT, "tests", "cpp", "new_map_points_two_cameras_harness.cpp"),
                        LIB, "-Wl,-rpath," + os.path.dirname(LIB), "-Wl,-rpath,/opt/rocm/lib", "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def table_bytes(t, pose15, nleft, two_cameras, uright=None, depth=None, key=None):
    n = len(t.node)
    uright = np.full(n, -1, f32) if uright is None else uright
    depth = np.full(n, -1, f32) if depth is None else depth
    key = np.zeros((n, 2), f32) if key is None else key
    return (np.array([n, nleft, int(two_cameras)], np.int32).tobytes() + np.asarray(pose15, f32).tobytes() + t.x.tobytes() +
            t.y.tobytes() + t.octave.tobytes() + t.angle.tobytes() + np.ascontiguousarray(t.desc).tobytes() + t.node.tobytes() +
            t.has_mp.tobytes() + np.asarray(uright, f32).tobytes() + np.asarray(depth, f32).tobytes() +
            np.ascontiguousarray(key, f32).tobytes())


def header(nkf, coarse, far, stop_before, cam_left, cam_right, par):
    return (np.array([nkf, int(coarse), int(far), stop_before], np.int32).tobytes() + np.asarray(cam_left, f32).tobytes() +
            np.asarray(cam_right, f32).tobytes() + np.hstack([two.TLR_R, two.TLR_T.reshape(3, 1)]).astype(f32).tobytes() +
            np.asarray(par, f32).tobytes())


def write_input(path, kf1, nbrs, coarse, far, stop_before):
    """Keyframes of two cameras (helpers_new_map_points_two_cameras KF / NB): the left side's 15 floats are the keyframe's pose."""
    with open(path, "wb") as f:
        f.write(header(len(nbrs), coarse, far, stop_before, two.CAMS[0], two.CAMS[1], (0.0, 0.0, h.TH_FAR, 1.2)))
        for kf in [kf1] + [nb.kf for nb in nbrs]:
            f.write(table_bytes(kf.t, kf.pose[0], kf.t.nleft, True))


def parse(path, n1):
    raw = np.fromfile(path, np.int32)
    created, nlog = int(raw[0]), int(raw[1])
    log = [tuple(int(v) for v in row) for row in raw[2:2 + 4 * nlog].reshape(nlog, 4)]
    rest = raw[2 + 4 * nlog:]
    return created, log, rest[:3 * created].view(f32).reshape(created, 3), rest[3 * created:]


@pytest.mark.gpu
@pytest.mark.parametrize("stop_before", [-1, 2])
def test_the_adapter_replays_the_loop_in_the_reference_order(tmp_path, oracle, stop_before):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    exe = build(str(tmp_path))
    kf1, nbrs, _ = h.scene(h.SEEDS[0])
    nbrs = nbrs[:4]
    nkf, n1 = len(nbrs), len(kf1.t.node)
    for coarse, far in ((False, True), (True, False)):
        inp, outp = str(tmp_path / "in"), str(tmp_path / "out")
        write_input(inp, kf1, nbrs, coarse, far, stop_before)
        r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        created, log, pos, tail = parse(outp, n1)
        order = []
        m, n, _, _, _ = h.create_new_map_points(oracle, kf1, nbrs, coarse, far, h.TH_FAR, order=order,
                                                stop_before=stop_before if stop_before > 0 else None)
        want, nwant = expected_log(order, nkf, stop_before)
        assert created == nwant and nwant > 0
        assert log == want, next((a, b) for a, b in zip(log, want) if a != b) if len(log) == len(want) else (len(log), len(want))
        assert np.array_equal(pos.view(np.uint32), np.array([o[3] for o in order], f32).view(np.uint32))
        # the sequence of single searches with the replay between them sees what the loop's searches see
        applied = stop_before if 0 < stop_before < nkf else nkf
        seq = tail[:applied * (n1 + 1)].reshape(applied, n1 + 1)
        for k in range(applied):
            assert seq[k, 0] == n[k] and np.array_equal(seq[k, 1:], m[k]), (k, int((seq[k, 1:] != m[k]).sum()))
        assert tail[applied * (n1 + 1):].tolist() == [1, 1], "the two refusals"
        if stop_before < 0:
            assert len({o[0] for o in order}) >= 2


@pytest.mark.gpu
def test_a_call_of_one_camera_keyframes_is_forwarded(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    exe = build(str(tmp_path))
    kf1, nbrs = H1.scene(21, 3, 300, nnodes=20, f12_zero=False)
    inp, outp = str(tmp_path / "in"), str(tmp_path / "out")
    cam8 = tuple(H1.CAM[:4]) + (0.0, 0.0, 0.0, 0.0)
    with open(inp, "wb") as f:
        f.write(header(len(nbrs), False, True, -1, cam8, cam8, (H1.CAM[4], H1.MB, 9.0, 1.2)))
        for kf in [kf1] + [nb.kf for nb in nbrs]:
            f.write(table_bytes(kf.t, kf.pose, -1, False, kf.uright, kf.depth, kf.key))
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    created, log, pos, tail = parse(outp, len(kf1.t.node))
    geo = tail.view(f32).reshape(len(nbrs), 11)
    mine = [nb._replace(F12=geo[k, :9].reshape(3, 3).copy(), ep=geo[k, 9:].copy()) for k, nb in enumerate(nbrs)]
    order = []
    H1.create_new_map_points(kf1, mine, far=True, th_far=9.0, order=order)
    want, nwant = expected_log(order, len(nbrs), -1)
    assert created == nwant and nwant > 0 and log == want
    assert np.array_equal(pos.view(np.uint32), np.array([o[3] for o in order], f32).view(np.uint32))


def test_the_harness_builds_and_fails_loudly_without_a_device(tmp_path):
    """Here (no GPU) the extractor call throws pli::Error(PLI_ERR_NO_DEVICE) and the harness exits with 1; on the GPU box the same
    program runs.  Either way PliCreateNewMapPointsTwoCameras compiles against the stub types and links against the library."""
    import torch
    exe = build(str(tmp_path))
    kf1, nbrs = h.w_zero_scene()
    inp, outp = str(tmp_path / "in"), str(tmp_path / "out")
    write_input(inp, kf1, nbrs, True, False, -1)
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300)
    if torch.cuda.is_available():
        assert r.returncode == 0, r.stderr
    else:
        assert r.returncode == 1 and "no HIP device" in r.stderr, (r.returncode, r.stderr)
