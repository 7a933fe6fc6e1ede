"""The C++ SearchByBoW adapters for a rig of two cameras, executed (-m gpu): tests/cpp/bow_two_cameras_harness.cpp calls
PliORBmatcherTwoCameras::SearchByBoW(pKF, F, vpMapPointMatches) per keyframe and the batch overload once, on stub KeyFrame / Frame
types holding std::map FeatureVectors.  Four cases: a two-camera frame against two-camera keyframes and against a keyframe of one
camera (pli_search_by_bow_two_cameras; the restatement of tests/test_bow_two_cameras_cpu.py), a one-camera frame against
two-camera keyframes (pli_search_by_bow with the keyframe's angles from mvKeys / mvKeysRight) and one-camera types throughout
(forwarded to PliORBmatcher; both: the restatement of tests/test_bow_search_cpu.py).  The dumped vpMapPointMatches (keyframe
feature indices) and return values equal the restatements."""
import os
import subprocess

import numpy as np
import pytest

from test_bow_search_cpu import keyframe_of, search_by_bow_fast
from test_bow_two_cameras_cpu import F_NLEFT, NNODES, make_frame, search_closed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "pli_slam_amd", "csrc", "libpli_frontend.so")


def build(outdir):
    exe = os.path.join(outdir, "bow_two_cameras_harness")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-pthread", "-I", ROOT, "-I", os.path.join(ROOT, "tests", "stubs"),
                        os.path.join(ROOT, "tests", "cpp", "bow_two_cameras_harness.cpp"), LIB, "-Wl,-rpath," + os.path.dirname(LIB),
                        "-Wl,-rpath,/opt/rocm/lib", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def write_input(path, frame, f_nleft, kfs, nnratio, check_orientation):
    """kfs: (desc, angle, node, state, nleft) per keyframe; f_nleft / nleft -1: one camera."""
    fd, fa, fn = frame
    with open(path, "wb") as f:
        f.write(np.array([len(kfs), len(fn), f_nleft], np.int32).tobytes() + np.float32(nnratio).tobytes() +
                np.int32(int(check_orientation)).tobytes())
        f.write(np.ascontiguousarray(fd, np.uint8).tobytes() + np.asarray(fa, np.float32).tobytes() + np.asarray(fn, np.int32).tobytes())
        for kd, ka, kn, state, nleft in kfs:
            f.write(np.array([len(kn), nleft], np.int32).tobytes() + np.ascontiguousarray(kd, np.uint8).tobytes() +
                    np.asarray(ka, np.float32).tobytes() + np.asarray(kn, np.int32).tobytes() + np.asarray(state, np.uint8).tobytes())


def make_case(rng, nkf, kf_two_cameras):
    frame = make_frame(rng)
    kfs = []
    for k in range(nkf):
        kd, ka, kn, _ = keyframe_of(rng, frame, int(rng.integers(150, 400)), nnodes=NNODES)
        state = rng.choice([0, 1, 1, 1, 2], len(kn)).astype(np.uint8)           # no map point / good / isBad()
        kfs.append((kd, ka, kn, state, int(rng.integers(0, len(kn) + 1)) if kf_two_cameras[k % len(kf_two_cameras)] else -1))
    return frame, kfs


CASES = (  # (frame of two cameras, keyframes of two cameras, ratio, orientation)
    (True, (True,), 0.7, True), (True, (False, True), 0.7, True), (False, (True,), 0.75, True), (False, (False,), 0.7, False),
    (True, (True, False), 0.9, False))


@pytest.mark.gpu
def test_two_camera_search_by_bow_adapters_equal_the_restatements(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    exe = build(str(tmp_path))
    rng = np.random.default_rng(31)
    for f_two, kf_two, ratio, ori in CASES:
        frame, kfs = make_case(rng, 3, kf_two)
        nf = len(frame[2])
        inp, outp = str(tmp_path / "in"), str(tmp_path / "out")
        write_input(inp, frame, F_NLEFT if f_two else -1, kfs, ratio, ori)
        r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        got = np.fromfile(outp, np.int32).reshape(2, len(kfs), nf + 1)
        total = right = 0
        for k, (kd, ka, kn, state, _) in enumerate(kfs):
            valid = (state == 1).astype(np.uint8)
            if f_two:
                want_m, want_n = search_closed(kd, ka, kn, valid, *frame, F_NLEFT, ratio, ori)
            else:
                want_m, want_n = search_by_bow_fast(kd, ka, kn, valid, *frame, ratio, ori)
            for call in range(2):                   # single call, then the batch call
                assert got[call, k, 0] == want_n, (f_two, kf_two, call, k, got[call, k, 0], want_n)
                assert np.array_equal(got[call, k, 1:], want_m), (f_two, kf_two, call, k)
            total += want_n
            right += int((want_m[F_NLEFT:] >= 0).sum())
        assert total > 0 and right > 0


def test_two_camera_search_by_bow_harness_builds_and_fails_loudly_without_a_device(tmp_path):
    """Here (no GPU) the extractor call throws pli::Error(PLI_ERR_NO_DEVICE) and the harness exits with 1; on the GPU box the
    same program runs.  Either way it builds and links against the product library."""
    import torch
    exe = build(str(tmp_path))
    frame, kfs = make_case(np.random.default_rng(1), 1, (True,))
    inp, outp = str(tmp_path / "in"), str(tmp_path / "out")
    write_input(inp, frame, F_NLEFT, kfs, 0.7, True)
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300)
    if torch.cuda.is_available():
        assert r.returncode == 0, r.stderr
    else:
        assert r.returncode == 1 and "no HIP device" in r.stderr, (r.returncode, r.stderr)
