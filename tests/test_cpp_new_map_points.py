"""The C++ adapter PliCreateNewMapPoints (pli_slam_amd/adapters/orbslam_local_mapping.hpp), executed (-m gpu):
tests/cpp/new_map_points_harness.cpp runs it on stub KeyFrame / MapPoint / Atlas types that log every call of
LocalMapping.cc:670-683; the dumped order of new MapPoint / AddObservation / AddMapPoint / ComputeDistinctiveDescriptors /
UpdateNormalAndDepth / Atlas::AddMapPoint calls, mlpRecentAddedMapPoints and the positions equal what the Python restatement of the
reference's loop (tests/helpers_new_map_points.py) creates, run on the F12 / epipole that the adapter's own geometry function
produced; with a CheckNewKeyFrames() that answers true before neighbour 2 they equal the restatement cut there."""
import os
import subprocess

import numpy as np
import pytest

import helpers_new_map_points as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "pli_slam_amd", "csrc", "libpli_frontend.so")
TH_FAR = 9.0


def build(outdir):
    exe = os.path.join(outdir, "new_map_points_harness")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", "-pthread", "-I", ROOT, "-I",
                        os.path.join(ROOT, "tests", "stubs"), os.path.join(ROOT, "tests", "cpp", "new_map_points_harness.cpp"),
                        LIB, "-Wl,-rpath," + os.path.dirname(LIB), "-Wl,-rpath,/opt/rocm/lib", "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def table_bytes(kf):
    t = kf.t
    return (np.int32(len(t.node)).tobytes() + np.asarray(kf.pose, np.float32).tobytes() + t.x.tobytes() + t.y.tobytes() +
            t.octave.tobytes() + t.angle.tobytes() + np.ascontiguousarray(t.desc).tobytes() + t.node.tobytes() + t.has_mp.tobytes() +
            kf.uright.tobytes() + kf.depth.tobytes() + np.ascontiguousarray(kf.key, np.float32).tobytes())


def write_input(path, kf1, nbrs, coarse, far, stop_before):
    with open(path, "wb") as f:
        f.write(np.array([len(nbrs), int(coarse), int(far), stop_before], np.int32).tobytes())
        f.write(np.array(H.CAM[:4] + (H.CAM[4], H.MB, TH_FAR, 1.2), np.float32).tobytes())
        f.write(table_bytes(kf1))
        for nb in nbrs:
            f.write(table_bytes(nb.kf))


def expected_log(order, nkf, stop_before):
    log = []
    serial = 0
    for k in range(nkf):
        if k > 0:
            log.append((7, k, 0, 0))
            if k == stop_before:
                break
        for kk, i, j, _ in order:
            if kk != k:
                continue
            log += [(0, 0, serial, 0), (1, serial, 0, i), (1, serial, k + 1, j), (2, 0, serial, i), (2, k + 1, serial, j),
                    (3, serial, 0, 0), (4, serial, 0, 0), (5, serial, 0, 0)]
            serial += 1
    return log + [(6, s, 0, 0) for s in range(serial)], serial


@pytest.mark.gpu
@pytest.mark.parametrize("stop_before", [-1, 2])
def test_the_adapter_replays_the_loop_in_the_reference_order(tmp_path, stop_before):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    exe = build(str(tmp_path))
    for seed, nkf, coarse, far in ((21, 5, False, True), (22, 3, True, False)):
        kf1, nbrs = H.scene(seed, nkf, 300, nnodes=20, f12_zero=False)
        inp, outp = str(tmp_path / "in"), str(tmp_path / "out")
        write_input(inp, kf1, nbrs, coarse, far, stop_before)
        r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        raw = np.fromfile(outp, np.int32)
        created, nlog = int(raw[0]), int(raw[1])
        log = [tuple(int(v) for v in row) for row in raw[2:2 + 4 * nlog].reshape(nlog, 4)]
        rest = raw[2 + 4 * nlog:].view(np.float32)
        pos, geo = rest[:3 * created].reshape(created, 3), rest[3 * created:].reshape(nkf, 11)
        mine = [nb._replace(F12=geo[k, :9].reshape(3, 3).copy(), ep=geo[k, 9:].copy()) for k, nb in enumerate(nbrs)]
        order = []
        H.create_new_map_points(kf1, mine, coarse=coarse, far=far, th_far=TH_FAR, order=order,
                                stop_before=stop_before if stop_before > 0 else None)
        want, nwant = expected_log(order, nkf, stop_before)
        assert created == nwant and nwant > 0
        assert log == want, next((a, b) for a, b in zip(log, want) if a != b) if len(log) == len(want) else (len(log), len(want))
        assert np.array_equal(pos.view(np.uint32), np.array([o[3] for o in order], np.float32).view(np.uint32))
        if stop_before < 0:
            assert len({o[0] for o in order}) >= 2


def test_the_harness_builds_and_fails_loudly_without_a_device(tmp_path):
    """Here (no GPU) the extractor call throws pli::Error(PLI_ERR_NO_DEVICE) and the harness exits with 1; on the GPU box the
    same program runs.  Either way PliCreateNewMapPoints compiles against the stub types and links against the product library."""
    import torch
    exe = build(str(tmp_path))
    kf1, nbrs = H.scene(1, 2, 40, nnodes=5)
    inp, outp = str(tmp_path / "in"), str(tmp_path / "out")
    write_input(inp, kf1, nbrs, False, False, -1)
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300)
    if torch.cuda.is_available():
        assert r.returncode == 0, r.stderr
    else:
        assert r.returncode == 1 and "no HIP device" in r.stderr, (r.returncode, r.stderr)
