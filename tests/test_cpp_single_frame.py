"""The C++ adapter of the single-camera Frame constructors (pli_slam_amd/adapters/frame_single.hpp), host only: the harness
tests/cpp/single_frame_harness.cpp, a stand-alone program with its own main, is built against tests/cpp/mock_pli_single_frame.cpp
(pli_frame_extract_single and pli_set_pinhole_distortion with made-up deterministic results) with -fsanitize=address,undefined and
run here.  It fills a stub Frame through PliSingleCameraFrame and compares every member with what the C entry point returned:
mvKeys, mDescriptors, monoLeft, mvKeys_Line, mDescriptors_Line, mvKeysUn (pt replaced, the other fields mvKeys'), mvKeysUn_Line,
mvuRight, mvDepth, the order of mGrid's cells, mnMinX .. mnMaxY on the first Frame only, the early return of a Frame without
keypoints, the k1 == 0 copies."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["rgbd first frame", "second frame keeps the bounds", "empty frame returns early", "monocular frame", "k1 == 0 copies", "bad arguments"]


def test_the_adapter_fills_a_stub_frame_under_address_and_ub_sanitizers(tmp_path):
    exe = str(tmp_path / "single_frame_harness")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                        "-pthread", "-I", ROOT, "-I", os.path.join(ROOT, "tests", "stubs"),
                        os.path.join(ROOT, "tests", "cpp", "single_frame_harness.cpp"),
                        os.path.join(ROOT, "tests", "cpp", "mock_pli_single_frame.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1 exitcode=66", UBSAN_OPTIONS="print_stacktrace=1 halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert lines == ["ok " + c for c in CASES] + ["all ok"], r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
