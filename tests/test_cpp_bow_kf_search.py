"""The C++ SearchByBoW(KF, KF) adapters, executed (-m gpu): tests/cpp/bow_kf_search_harness.cpp calls
PliORBmatcher::SearchByBoW(pKF1, pKF2, vpMatches12) per pair and the batch overload once, on stub KeyFrame types holding std::map
FeatureVectors and map points that are missing, good or bad on both sides; the dumped vpMatches12 (feature indices of pKF2) and
return values equal the Python restatement of ORBmatcher.cc:823-963 (tests/test_bow_kf_search_cpu.py)."""
import os
import subprocess

import numpy as np
import pytest

from test_bow_search_cpu import keyframe_of, random_case
from test_bow_kf_search_cpu import search_by_bow_kf_fast

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "pli_slam_amd", "csrc", "libpli_frontend.so")


def build(outdir):
    exe = os.path.join(outdir, "bow_kf_search_harness")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-pthread", "-I", ROOT, "-I", os.path.join(ROOT, "tests", "stubs"),
                        os.path.join(ROOT, "tests", "cpp", "bow_kf_search_harness.cpp"), LIB, "-Wl,-rpath," + os.path.dirname(LIB),
                        "-Wl,-rpath,/opt/rocm/lib", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def write_input(path, kf1, kfs, nnratio, check_orientation):
    with open(path, "wb") as f:
        f.write(np.int32(len(kfs)).tobytes() + np.float32(nnratio).tobytes() + np.int32(int(check_orientation)).tobytes())
        for kd, ka, kn, state in [kf1] + list(kfs):
            f.write(np.int32(len(kn)).tobytes() + np.ascontiguousarray(kd, np.uint8).tobytes() + np.asarray(ka, np.float32).tobytes() +
                    np.asarray(kn, np.int32).tobytes() + np.asarray(state, np.uint8).tobytes())


def states(rng, n):
    return rng.choice([0, 1, 1, 1, 2], n).astype(np.uint8)                  # no map point / good / isBad()


@pytest.mark.gpu
def test_search_by_bow_kf_adapters_equal_the_restatement(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    exe = build(str(tmp_path))
    rng = np.random.default_rng(31)
    for n1, nnodes, ratio, ori in ((500, 25, 0.75, True), (300, 1, 0.7, True), (600, 60, 0.7, False)):
        d1, a1, nd1, _, _, _, _ = random_case(rng, n1, 1, nnodes, ndup=0.5)
        kf1 = (d1, a1, nd1, states(rng, n1))
        kfs = []
        for k in range(6):
            kd, ka, kn, _ = keyframe_of(rng, (d1, a1, nd1), int(rng.integers(0, 600)), nnodes=nnodes)
            kfs.append((kd, ka, kn, states(rng, len(kn))))
        inp, outp = str(tmp_path / "in"), str(tmp_path / "out")
        write_input(inp, kf1, kfs, ratio, ori)
        r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        got = np.fromfile(outp, np.int32).reshape(2, len(kfs), n1 + 1)
        total = 0
        for k, (kd, ka, kn, state) in enumerate(kfs):
            want_m, want_n = search_by_bow_kf_fast(d1, a1, nd1, (kf1[3] == 1).astype(np.uint8), kd, ka, kn,
                                                   (state == 1).astype(np.uint8), ratio, ori)
            for call in range(2):                   # single call, then the batch call
                assert got[call, k, 0] == want_n, (call, k, got[call, k, 0], want_n)
                assert np.array_equal(got[call, k, 1:], want_m), (call, k)
            total += want_n
        assert total > 0


def test_search_by_bow_kf_harness_builds_and_fails_loudly_without_a_device(tmp_path):
    """Here (no GPU) the extractor call throws pli::Error(PLI_ERR_NO_DEVICE) and the harness exits with 1; on the GPU box the
    same program runs.  Either way it builds and links against the product library."""
    import torch
    exe = build(str(tmp_path))
    rng = np.random.default_rng(1)
    d1, a1, nd1, _, _, _, _ = random_case(rng, 50, 1, 5)
    kd, ka, kn, _, _, _, _ = random_case(rng, 40, 1, 5)
    inp, outp = str(tmp_path / "in"), str(tmp_path / "out")
    write_input(inp, (d1, a1, nd1, np.ones(50, np.uint8)), [(kd, ka, kn, np.ones(40, np.uint8))], 0.75, True)
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300)
    if torch.cuda.is_available():
        assert r.returncode == 0, r.stderr
    else:
        assert r.returncode == 1 and "no HIP device" in r.stderr, (r.returncode, r.stderr)
