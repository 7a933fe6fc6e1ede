"""The C++ SearchByBoW(KF, KF) members of PliORBmatcherTwoCameras, executed (-m gpu): tests/cpp/bow_kf_two_cameras_harness.cpp calls
the single form per pair and the batch form once on stub keyframes with NLeft != -1 and mvKeysUn shorter than N, and then the base
matcher (PliORBmatcher) on copies of the keyframes cut to their first mvKeysUn.size() rows; the two dumps are equal, and equal the
literal restatement of tests/test_bow_kf_two_cameras_cpu.py.  Keyframes of one camera are forwarded."""
import os
import subprocess

import numpy as np
import pytest

from test_bow_kf_two_cameras_cpu import cases, search_literal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "pli_slam_amd", "csrc", "libpli_frontend.so")


def build(outdir):
    exe = os.path.join(outdir, "bow_kf_two_cameras_harness")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-pthread", "-I", ROOT, "-I", os.path.join(ROOT, "tests", "stubs"),
                        os.path.join(ROOT, "tests", "cpp", "bow_kf_two_cameras_harness.cpp"), LIB, "-Wl,-rpath," + os.path.dirname(LIB),
                        "-Wl,-rpath,/opt/rocm/lib", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def write_input(path, kf1, kfs, nnratio, check_orientation):
    """state: 0 = no map point, 1 = good, 2 = isBad() (every third flag that is off)."""
    with open(path, "wb") as f:
        f.write(np.int32(len(kfs)).tobytes() + np.float32(nnratio).tobytes() + np.int32(int(check_orientation)).tobytes())
        for d, a, nd, good, nleft, nun in [kf1] + list(kfs):
            n = len(nd)
            state = np.where(np.asarray(good) != 0, 1, np.where(np.arange(n) % 3 == 0, 2, 0)).astype(np.uint8)
            f.write(np.array([n, nun, nleft], np.int32).tobytes() + np.ascontiguousarray(d, np.uint8).tobytes() +
                    np.asarray(a, np.float32).tobytes() + np.asarray(nd, np.int32).tobytes() + state.tobytes())


@pytest.mark.gpu
def test_the_hidden_members_equal_the_base_on_cut_keyframes_and_the_restatement(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    exe = build(str(tmp_path))
    total = 0
    for (kf1, kfs), (ratio, ori) in zip(cases()[::2], ((0.75, True), (0.7, False)) * 8):
        inp, outp = str(tmp_path / "in"), str(tmp_path / "out")
        write_input(inp, kf1, kfs, ratio, ori)
        r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        n1 = len(kf1[2])
        got = np.fromfile(outp, np.int32).reshape(4, len(kfs), n1 + 1)       # two-camera single, batch; base on the cuts single, batch
        for k, kf2 in enumerate(kfs):
            want_m, want_n = search_literal(kf1, kf2, ratio, ori)
            for call in range(4):
                assert got[call, k, 0] == want_n, (call, k, got[call, k, 0], want_n)
                assert np.array_equal(got[call, k, 1:], want_m), (call, k)
            total += want_n
    assert total > 0
