"""The C++ SearchForTriangulation adapters, executed (-m gpu): tests/cpp/triangulation_search_harness.cpp calls
PliORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo, bCoarse) per neighbour and the batch form
once, on stub KeyFrame types holding std::map FeatureVectors and poses; the dumped pair lists and return values equal the
Python restatement of ORBmatcher.cc:965-1206 (tests/test_triangulation_search_cpu.py) run on the F12 / epipole that the adapter's
own geometry function (pli_detail::triangulationGeometry) produced - the host arithmetic is OpenCV's in the reference and is
not pinned here, so it is taken as given and checked only for being a fundamental matrix of the poses (to float accuracy)."""
import os
import subprocess

import numpy as np
import pytest

from test_triangulation_search_cpu import K_EUROC, geometry_np, search_for_triangulation_fast, two_view_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "pli_slam_amd", "csrc", "libpli_frontend.so")


def build(outdir):
    exe = os.path.join(outdir, "triangulation_search_harness")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", "-pthread", "-I", ROOT, "-I",
                        os.path.join(ROOT, "tests", "stubs"), os.path.join(ROOT, "tests", "cpp", "triangulation_search_harness.cpp"),
                        LIB, "-Wl,-rpath," + os.path.dirname(LIB), "-Wl,-rpath,/opt/rocm/lib", "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def table_bytes(t, R, tr):
    return (np.int32(len(t.node)).tobytes() + np.asarray(R, np.float32).tobytes() + np.asarray(tr, np.float32).tobytes() +
            t.x.tobytes() + t.y.tobytes() + t.octave.tobytes() + t.angle.tobytes() + np.ascontiguousarray(t.desc).tobytes() +
            t.node.tobytes() + t.has_mp.tobytes() + t.stereo.tobytes())


def write_input(path, t1, nbrs, poses, only_stereo, coarse, ori):
    with open(path, "wb") as f:
        f.write(np.array([len(nbrs), int(only_stereo), int(coarse), int(ori)], np.int32).tobytes())
        f.write(np.asarray(K_EUROC, np.float32).tobytes())
        f.write(table_bytes(t1, poses[0][0], poses[0][1]))
        for nb, p in zip(nbrs, poses):
            f.write(table_bytes(nb[0], p[2], p[3]))


@pytest.mark.gpu
def test_search_for_triangulation_adapters_equal_the_restatement(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    exe = build(str(tmp_path))
    rng = np.random.default_rng(31)
    for nkf, npts, nnodes, only_stereo, coarse, ori in ((5, 400, 25, False, False, False), (3, 300, 2, True, False, True),
                                                        (4, 500, 40, False, True, True)):
        poses = []
        t1, nbrs = two_view_case(rng, nkf, npts, nnodes, poses=poses)
        inp, outp = str(tmp_path / "in"), str(tmp_path / "out")
        write_input(inp, t1, nbrs, poses, only_stereo, coarse, ori)
        r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        n1 = len(t1.node)
        raw = np.fromfile(outp, np.int32)
        got = raw[:2 * nkf * (n1 + 1)].reshape(2, nkf, n1 + 1)
        geo = raw[2 * nkf * (n1 + 1):].view(np.float32).reshape(nkf, 11)
        total = 0
        for k, (t2, _, _, truth) in enumerate(nbrs):
            F12, ep = geo[k, :9].reshape(3, 3), geo[k, 9:]
            # the adapter's matrix is the fundamental matrix of the two poses up to float rounding
            Fd, epd = geometry_np(*[np.asarray(a, np.float32).astype(np.float64) for a in poses[k]])
            assert np.abs(F12 - Fd).max() <= 1e-4 * np.abs(Fd).max() and np.abs(ep - epd).max() < 0.05
            want_m, want_n = search_for_triangulation_fast(t1, t2, F12, ep, only_stereo, coarse, ori)
            for call in range(2):                   # single calls, then the batch call
                assert got[call, k, 0] == want_n, (call, k, got[call, k, 0], want_n)
                assert np.array_equal(got[call, k, 1:], want_m), (call, k)
            total += want_n
            if not coarse:
                assert ((want_m == truth) & (truth >= 0)).sum() > 0
        assert total > 0


def test_search_for_triangulation_harness_builds_and_fails_loudly_without_a_device(tmp_path):
    """Here (no GPU) the extractor call throws pli::Error(PLI_ERR_NO_DEVICE) and the harness exits with 1; on the GPU box the
    same program runs.  Either way it builds and links against the product library."""
    import torch
    exe = build(str(tmp_path))
    poses = []
    t1, nbrs = two_view_case(np.random.default_rng(1), 2, 40, 5, poses=poses)
    inp, outp = str(tmp_path / "in"), str(tmp_path / "out")
    write_input(inp, t1, nbrs, poses, False, False, True)
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300)
    if torch.cuda.is_available():
        assert r.returncode == 0, r.stderr
    else:
        assert r.returncode == 1 and "no HIP device" in r.stderr, (r.returncode, r.stderr)
