"""The C++ head of Tracking::GrabImage* (pli_slam_amd/adapters/tracking_grab.hpp) and PliSingleCameraFrame::extractRaw, host only: the
harness tests/cpp/grab_image_harness.cpp, a stand-alone program with its own main, is built against tests/cpp/mock_pli.cpp plus its own
stand-ins for pli_set_image_format, pli_set_depth_format and pli_frame_extract_single (they record their arguments) with
-fsanitize=address,undefined and run here.  It checks the image format chosen for 1, 3 and 4 channels with and without mbRGB
(Tracking.cc:889-914), that 2 channels throw, that the setters are called only on a change, the gate of Tracking.cc:979 on four depth
maps, and that extractRaw hands pointers and strides on untouched."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["format for 1, 3 and 4 channels", "2 channels throw", "setters called only on change", "depth gate of Tracking.cc:979",
         "extractRaw forwards pointers and strides"]


def test_grab_image_picks_the_formats_and_extract_raw_forwards_under_address_and_ub_sanitizers(tmp_path):
    exe = str(tmp_path / "grab_image_harness")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                        "-pthread", "-I", ROOT, "-I", os.path.join(ROOT, "tests", "stubs"),
                        os.path.join(ROOT, "tests", "cpp", "grab_image_harness.cpp"),
                        os.path.join(ROOT, "tests", "cpp", "mock_pli.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1 exitcode=66", UBSAN_OPTIONS="print_stacktrace=1 halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert lines == ["ok " + c for c in CASES] + ["all ok"], r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
